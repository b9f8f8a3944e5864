"""Shared by the tests of the discriminator's 4 x 4 convolution on the fp16 matrix pipe (csrc/disc_conv.hip, networks/disc_conv.py;
test_disc_conv_cpu.py, test_disc_conv_gpu.py): a pure-Python mirror of the plan of include/pixelsynth_disc_conv.h, the formulas the
kernels evaluate (the adjoint as four parity gathers, the weight gradient) and the fp64 references under the two rules of
tests/_conv_bwd_ref.py, whose split, scale_of, measure and check are used as they are.  No test in here.

The measure.  sw = scale_of(max |w|), ws = w * sw with its split (wh, wl); sg = scale_of(max |g|), gs = g * sg with (gh, gl); (xh, xl)
the split of x.  Per result
    T    the three products the kernels sum, in fp64, divided by the scales     y: wl xh + wh xl + wh xh     gx: wl gh + wh gl + wh gh
                                                                                 gw: gl xh + gh xl + gh xh
    S    the same with the absolute values of the hi parts alone
    y32  torch's fp32 evaluation on the CPU of the three products in one call
    g64  the unsplit fp64 result, E32 = max |torch's plain fp32 evaluation on the CPU - g64|
and rule 1: |y - T| / S <= 10 |y32 - T| / S, rule 2: |y - g64| <= 4 max(E32, 1e-6 max |g64|), for the forward too.
"""
import functools
from collections import namedtuple

import torch
import torch.nn.functional as F

from _conv_bwd_ref import Gradient, check, measure, scale_of, split  # noqa: F401  (the tests take them from here)

PAD = 2
# (B, Ci, Co, H, W, stride): the issue's shapes -- a map smaller than the padding, odd and even sides at both strides, a tile plus a
# remainder on both axes, several channel blocks on either side --
SHAPES = [(1, 64, 64, 1, 1, 1), (2, 64, 128, 5, 7, 2), (1, 128, 64, 9, 11, 1), (3, 64, 64, 33, 34, 2), (1, 64, 64, 33, 33, 1),
          (2, 128, 256, 17, 17, 2), (1, 256, 512, 4, 5, 1)]
# and what the kernels' own branches need (test_disc_conv_cpu.py asserts each reaches its branch)
BRANCH_SHAPES = [(5, 256, 512, 13, 13, 1)]     # steps per part above the minimum (9), 64 channel blocks, parts that straddle frames
ALL_SHAPES = SHAPES + BRANCH_SHAPES


# ---- the plan (include/pixelsynth_disc_conv.h) ---------------------------------------------------------------------------------------------
MAX_PARTS, TARGET_WGS, MIN_CHUNK = 256, 512, 8
Plan = namedtuple("Plan", "Ho Wo Wo8 nch Q spf steps blocks chunk parts last straddle odd_tail pixel_groups launches")


def plan(B, Ci, Co, H, W, stride, pad=PAD):
    Ho, Wo = (H + 2 * pad - 4) // stride + 1, (W + 2 * pad - 4) // stride + 1
    Wo8 = -(-Wo // 8) * 8
    nch = Wo8 // 8
    Q = Ho * nch
    spf = -(-Q // 2)
    steps = B * spf
    blocks = (Co // 64) * (Ci // 32)
    chunk = max(MIN_CHUNK, -(-steps // min(MAX_PARTS, -(-TARGET_WGS // blocks))))
    ranges = [(t, min(t + chunk, steps)) for t in range(0, steps, chunk)]
    # grad_x's launches, (Hm, Wm) each: the frame at stride 1, the four parities (py, px) of the input pixel at stride 2
    launches = [(H, W)] if stride == 1 else [((H - py + 1) // 2, (W - px + 1) // 2) for py in range(2) for px in range(2)]
    return Plan(Ho, Wo, Wo8, nch, Q, spf, steps, blocks, chunk, len(ranges), ranges[-1][1] - ranges[-1][0],
                [i for i, (lo, hi) in enumerate(ranges) if lo // spf != (hi - 1) // spf], Q % 2 == 1, -(-(Ho * Wo) // 256), launches)


# ---- the route cases (test_disc_routes_cpu.py asserts each reaches its branches and no shape of ALL_SHAPES does; test_disc_routes_gpu.py
# runs them) --------------------------------------------------------------------------------------------------------------------------------
# name -> predicate over (shape, plan(*shape)), each the kernel's own line restated
BRANCHES = {
    # make_plan: `if (want > PS_DISC_CONV_MAX_PARTS) want = PS_DISC_CONV_MAX_PARTS` decides, and k_disc_conv_gw_sum adds 256 parts
    "parts-cap": lambda s, p: p.parts == MAX_PARTS,
    # the workload's plan in small: steps per part from ceil(steps / want) above the 8 and 9 of the operator shapes, over a hundred parts
    # for k_disc_conv_gw_sum, a shorter last part, parts in two frames, the product's grid of many pixel workgroups
    "workload-plan": lambda s, p: p.chunk >= 10 and p.parts > 100 and 1 < p.last < p.chunk and len(p.straddle) >= 3 and p.pixel_groups > 16,
    # k_disc_conv_gw_parts: `st1 = min(st0 + a.chunk, a.steps)` leaves the last of several parts one step
    "one-step-part": lambda s, p: p.parts > 1 and p.last == 1,
    # k_disc_conv_mfma: Cin / 16 = 32 channel steps per tap; k_disc_conv_gw_parts: ncib = 16; k_disc_conv_pack: n_in = 512 (forward)
    "ci-512": lambda s, p: s[1] == 512,
    # k_disc_conv_rows: `if (jj < Wo && ...)` holds for every j of every chunk: no row has a zero tail
    "wo-mult-8": lambda s, p: p.Wo % 8 == 0,
    # ... and for one j of a row's last chunk: seven zeros behind one value.  At stride 2 the operator shape (2, 128, 256, 17, 17, 2) has
    # Wo = 9 already (x = 2 jj + kx - 2 of k_disc_conv_rows); what no test runs is that row at stride 1, where the last chunk's one value
    # reads x[W - 2 + kx], past the frame for kx >= 2
    "wo-one-over": lambda s, p: p.Wo % 8 == 1 and s[5] == 1,
    # launch_conv: `if (a.Hm <= 0 || a.Wm <= 0) return PS_OK`
    "empty-parity": lambda s, p: any(hm <= 0 or wm <= 0 for hm, wm in p.launches),
    # ps_disc_conv_backward_f16x3: the launches of py = 1 write the rows 1, 3 .. H - 1: the frame's last row belongs to them
    "even-h-stride-2": lambda s, p: s[5] == 2 and s[3] % 2 == 0,
}
# (B, Ci, Co, H, W, stride) -> the branches the case is there for
ROUTES = {
    (16, 64, 64, 47, 41, 1): ("parts-cap",),                     # 2304 steps, 9 per part, exactly 256 parts
    (4, 64, 128, 129, 129, 2): ("workload-plan",),               # 118 parts of 10, the last of 2, parts 29 / 58 / 87 in two frames, 17 pixel
                                                                 # workgroups, parity launches of 65 and 64 rows
    (1, 64, 64, 16, 5, 1): ("one-step-part",),                   # 9 steps, 2 parts, the last of one step, a zero chunk behind the frame
    (1, 512, 64, 5, 5, 1): ("ci-512",),
    (1, 512, 512, 3, 3, 2): ("ci-512",),
    (2, 512, 128, 9, 10, 1): ("ci-512",),                        # ... with 3 parts, one in two frames
    (2, 64, 64, 6, 7, 1): ("wo-mult-8",),                        # Wo = 8 at stride 1
    (1, 64, 64, 9, 15, 2): ("wo-mult-8",),                       # Wo = 8 at stride 2
    (1, 64, 64, 3, 8, 1): ("wo-one-over",),                      # Wo = 9, Wo8 = 16
    (2, 64, 64, 1, 1, 2): ("empty-parity",),                     # three of the four launches are empty
    (1, 64, 64, 1, 6, 2): ("empty-parity",),
    (1, 64, 64, 4, 1, 2): ("empty-parity", "even-h-stride-2"),
    (1, 64, 64, 4, 6, 2): ("even-h-stride-2",),
    (1, 64, 64, 2, 2, 2): ("even-h-stride-2",),
}
ROUTE_SHAPES = list(ROUTES)
ABI_SHAPES = [(16, 64, 64, 47, 41, 1), (1, 512, 512, 3, 3, 2), (1, 64, 64, 3, 8, 1), (2, 64, 64, 1, 1, 2)]      # through the C ABI inside rims
TINY_SHAPE, TINY_EXPONENTS = (2, 64, 64, 5, 7, 2), (8, 16, -115)       # the gradient under the held exponent: x 2^8, w 2^16, g 2^-115


def workspace_bytes(B, Ci, Co, H, W, stride, pad=PAD):
    """make_plan's regions in their order, each rounded up to 256 bytes -> (bytes, the offset of the parts, the bytes of the parts)"""
    p = plan(B, Ci, Co, H, W, stride, pad)
    Hp, Wp = H + 2 * pad, W + 2 * pad
    halves = [16 * Co * Ci, B * Hp * Wp * Ci, B * (p.Ho + 2) * (p.Wo + 2) * Co, B * Co * p.Ho * p.Wo8, 4 * B * Ci * Hp * p.Wo8]
    part = p.parts * 16 * Co * Ci * 4
    regions = [256 * 4, 2 * 4] + [4 * n for n in halves] + [part]
    at = 0
    for n in regions[:-1]:
        at += -(-n // 256) * 256
    return at + -(-part // 256) * 256, at, part


# ---- the formulas --------------------------------------------------------------------------------------------------------------------------
def conv(x, w, stride):
    return F.conv2d(x, w, None, stride, PAD)


def grad_input(g, w, stride, H, W):
    """The adjoint of conv in x as the kernels evaluate it, a gather: at stride 1 the convolution of g (padding 1) with the flipped,
    transposed weight; at stride 2 four 2 x 2 stride-1 products, one per parity (py, px) of the input pixel -- input pixel (2 m + py,
    2 n + px) sums g[m + ty, n + tx] w[py + 2 (1 - ty), px + 2 (1 - tx)] over ty, tx in {0, 1}, g zero outside its frame."""
    if stride == 1:
        return F.conv2d(g, w.flip(2, 3).transpose(0, 1), None, 1, 1)
    out = g.new_zeros(g.size(0), w.size(1), H, W)
    gp = F.pad(g, (0, 1, 0, 1))
    for py in range(2):
        for px in range(2):
            Hm, Wm = (H - py + 1) // 2, (W - px + 1) // 2
            if Hm == 0 or Wm == 0:
                continue
            sub = w[:, :, [py + 2, py]][:, :, :, [px + 2, px]].transpose(0, 1)      # [c, o, ty, tx]
            out[:, :, py::2, px::2] = F.conv2d(gp, sub)[:, :, :Hm, :Wm]
    return out


def grad_weight(x, g, stride):
    """sum_{b,oy,ox} g[b,o,oy,ox] xpad[b,c,oy stride + ky, ox stride + kx] -> (Co, Ci, 4, 4): the batch as the channels of a dilated
    convolution of xpad with g as its kernel"""
    xp = F.pad(x, (PAD,) * 4)
    return F.conv2d(xp.transpose(0, 1), g.transpose(0, 1), None, 1, 0, stride)[:, :, :4, :4].transpose(0, 1).contiguous()


# ---- the references ------------------------------------------------------------------------------------------------------------------------
Reference = namedtuple("Reference", "y x weight sg sw")


def reference(x, w, g, stride):
    """x (B, Ci, H, W), w (Co, Ci, 4, 4), g = grad_y, fp32 on the CPU -> Reference of Gradients for y, grad_x and grad_weight"""
    d = torch.double
    H, W = x.shape[2:]
    sg, sw = scale_of(g.abs().max().item()), scale_of(w.abs().max().item())
    gh, gl = split(g * sg)
    wh, wl = split(w * sw)
    xh, xl = split(x)
    leaves = [t.clone().requires_grad_() for t in (x, w)]
    y32 = conv(leaves[0], leaves[1], stride)
    g32 = torch.autograd.grad(y32, leaves, g)
    y64 = conv(x.to(d), w.to(d), stride)
    gx64, gw64 = grad_input(g.to(d), w.to(d), stride, H, W), grad_weight(x.to(d), g.to(d), stride)
    fwd = Gradient((conv(xh.to(d), wh.to(d) + wl.to(d), stride) + conv(xl.to(d), wh.to(d), stride)) / sw,
                   conv(xh.abs().to(d), wh.abs().to(d), stride) / sw,
                   conv(torch.cat([xh, xl, xh], 1), torch.cat([wh, wh, wl], 1), stride) / sw, y64,
                   (y32.detach().to(d) - y64).abs().max().item())
    gx = Gradient((grad_input(gh.to(d), wh.to(d) + wl.to(d), stride, H, W) + grad_input(gl.to(d), wh.to(d), stride, H, W)) / (sg * sw),
                  grad_input(gh.abs().to(d), wh.abs().to(d), stride, H, W) / (sg * sw),
                  grad_input(torch.cat([gh, gl, gh], 1), torch.cat([wh, wh, wl], 0), stride, H, W) / (sg * sw), gx64,
                  (g32[0].to(d) - gx64).abs().max().item())
    gw = Gradient((grad_weight(xh.to(d) + xl.to(d), gh.to(d), stride) + grad_weight(xh.to(d), gl.to(d), stride)) / sg,
                  grad_weight(xh.abs().to(d), gh.abs().to(d), stride) / sg,
                  grad_weight(torch.cat([xh, xl, xh]), torch.cat([gh, gh, gl]), stride) / sg, gw64,
                  (g32[1].to(d) - gw64).abs().max().item())
    return Reference(fwd, gx, gw, sg, sw)


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
def out_shape(B, Ci, Co, H, W, stride):
    return B, Co, (H + 2 * PAD - 4) // stride + 1, (W + 2 * PAD - 4) // stride + 1


def _gen(shape, seed):
    B, Ci, Co, H, W, stride = shape
    return torch.Generator().manual_seed(4321 + seed + 7 * Ci + Co + 13 * H + W + stride)


@functools.lru_cache(maxsize=None)
def integers(shape):
    """x and g in [-3, 3], w in [-2, 2]: every product and sum is exact in fp16, fp32 and fp64, under the power-of-two scales too
    -> x, w, g and the fp64 convolution's y, grad_x, grad_weight as fp32"""
    B, Ci, Co, H, W, stride = shape
    gen = _gen(shape, 0)
    x = torch.randint(-3, 4, (B, Ci, H, W), generator=gen).float()
    w = torch.randint(-2, 3, (Co, Ci, 4, 4), generator=gen).float()
    g = torch.randint(-3, 4, out_shape(*shape), generator=gen).float()
    leaves = [x.double().requires_grad_(), w.double().requires_grad_()]
    y = conv(leaves[0], leaves[1], stride)
    gx, gw = torch.autograd.grad(y, leaves, g.double())
    return x, w, g, y.detach().float(), gx.float(), gw.float()


def scaled_integers(shape, ex, ew, eg):
    """integers(shape) with x times 2^ex, w times 2^ew, g times 2^eg: powers of two, so every operand and the fp64 results times
    2^(ex + ew), 2^(ew + eg), 2^(ex + eg) are the exact ones -> the same six tensors as fp32.  Asserts what the comparison bit for bit
    rests on: each fp64 value survives the way through fp32, and none of them is a subnormal fp32."""
    x, w, g, y, gx, gw = integers(shape)
    d, tiny = torch.double, torch.finfo(torch.float32).tiny
    out = []
    for t, e in ((x, ex), (w, ew), (g, eg), (y, ex + ew), (gx, ew + eg), (gw, ex + eg)):
        t64 = t.to(d) * 2.0 ** e
        t32 = t64.float()
        assert torch.equal(t32.to(d), t64) and torch.equal(t32.to(d) * 2.0 ** -e, t.to(d)), e
        assert t32.any() and (t64[t64 != 0].abs() >= tiny).all() and torch.isfinite(t32).all(), e
        out.append(t32)
    return tuple(out)


def inputs(shape, seed=1, g_scale=1.0):
    """x = leaky_relu(randn), w = randn / sqrt(16 Ci), g = g_scale randn; deterministic, on the CPU"""
    B, Ci, Co, H, W, stride = shape
    gen = _gen(shape, seed)
    x = F.leaky_relu(torch.randn(B, Ci, H, W, generator=gen), 0.2)
    w = torch.randn(Co, Ci, 4, 4, generator=gen) / (16 * Ci) ** 0.5
    g = torch.randn(out_shape(*shape), generator=gen) * g_scale
    return x, w, g


def small_gradients(shape):
    """g = 1e-7 randn, one region a further 1e-3 smaller"""
    x, w, g = inputs(shape, seed=2, g_scale=1e-7)
    g[:, : g.size(1) // 2, : (g.size(2) + 1) // 2] *= 1e-3
    return x, w, g
