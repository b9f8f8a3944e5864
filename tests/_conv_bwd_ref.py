"""Shared by the tests of the split-fp16 convolution's backward pass (csrc/conv_bwd.hip, networks/f16x3.py:conv3x3_train;
test_conv_bwd_cpu.py, test_conv_bwd_gpu.py): the scale rule, a pure-Python mirror of the split of the reduction into parts, the fp64
references of what the kernels compute and the two assertions every gradient is held to.  No test in here.

The measure.  With s = scale_of(max |g|), gs = g * s and the splits (gh, gl) of gs, (xh, xl) of x, (wh, wl) of w (the forward's split,
_conv_f16x3_ref.split), per gradient:
    T    the three products the kernels sum -- gh * xh + gh * xl + gl * xh (weight), gh * wh + gh * wl + gl * wh (input) -- in fp64, / s
    S    the same with the absolute values of the hi parts alone: per element, the size of what was summed
    y32  torch's fp32 evaluation on the CPU of the three products in one call: exact fp32 products, another order
    g64  the unsplit fp64 gradient
    E32  max |torch's plain fp32 backward on the CPU - g64|
(the bias' gradient has no split: T = g64 = the fp64 sum of g, S = the sum of |g|, y32 = torch's fp32 sum) and
    1.  max |y - T| / S <= K16 * max |y32 - T| / S        K16 = 10: the margin _conv_f16x3_ref gives "another order"
    2.  max |y - g64|   <= 4 * max(E32, 1e-6 * max |g64|)  the rule of the splat backward's tests
check() prints error / bound for both before it asserts.
"""
import math
from collections import namedtuple

import torch
import torch.nn.functional as F

from _conv_f16x3_ref import K16, split

# ---- the scale rule (include/pixelsynth_conv_bwd.h) ----------------------------------------------------------------------------------------
def scale_of(m):
    """s for max |g| = m (a Python float holding an fp32 value): 2^(15 - e) with m = f * 2^e, f in [0.5, 1), the exponent held in
    [-126, 126]; 1 for 0, inf and NaN"""
    if not (m > 0 and m < math.inf):
        return 1.0
    e = math.frexp(m)[1]
    return 2.0 ** max(-126, min(126, 15 - e))


# ---- the split of the pixels into parts (csrc/conv_bwd.hip: make_plan) ----------------------------------------------------------------------
TILE_ROWS, TILE_COLS, BLOCK = 4, 16, 64      # a pixel tile; channels of either operand per workgroup
TARGET_WGS, MIN_CHUNK, MAX_PARTS = 512, 8, 256


def tiles(B, H, W):
    return B * (H // TILE_ROWS) * (W // TILE_COLS)


def part_ranges(B, H, W, Ci, Co):
    """[(first tile, one past the last tile)] of the parts, in order"""
    n = tiles(B, H, W)
    blocks = (Co // BLOCK) * (Ci // BLOCK)
    want = min(-(-TARGET_WGS // blocks), MAX_PARTS)
    chunk = max(-(-n // want), MIN_CHUNK)
    return [(t, min(t + chunk, n)) for t in range(0, n, chunk)]


PREP_BLOCKS, PREP_MIN_PIXELS = 256, 64      # the pass over g: ranges at most, pixels of a range at least

ConvPlan = namedtuple("ConvPlan", "tiles per_frame blocks chunk parts last straddle npix pchunk nprep ncb")


def plan(B, H, W, Ci, Co):
    """make_plan of csrc/conv_bwd.hip (the header states the formulas): tiles, tiles of a frame, 64 x 64 channel blocks, tiles per part
    (chunk), parts, tiles of the last part, the parts whose tiles lie in two frames; of the pass over g: pixels, pixels per range
    (pchunk), ranges (nprep), 64-channel blocks of Co (one maximum per range and block)"""
    rs = part_ranges(B, H, W, Ci, Co)
    per_frame = (H // TILE_ROWS) * (W // TILE_COLS)
    npix = B * H * W
    pchunk = max(-(-npix // PREP_BLOCKS), PREP_MIN_PIXELS)
    blocks = (Co // BLOCK) * (Ci // BLOCK)
    chunk = max(-(-tiles(B, H, W) // min(-(-TARGET_WGS // blocks), MAX_PARTS)), MIN_CHUNK)
    assert all(hi - lo == chunk for lo, hi in rs[:-1])
    return ConvPlan(tiles(B, H, W), per_frame, blocks, chunk, len(rs), rs[-1][1] - rs[-1][0],
                    [i for i, (lo, hi) in enumerate(rs) if lo // per_frame != (hi - 1) // per_frame],
                    npix, pchunk, -(-npix // pchunk), Co // BLOCK)


# ---- the references ---------------------------------------------------------------------------------------------------------------------------
def wgrad(x, g):
    """sum_{b,y,x} g[b,o,y,x] * xpad[b,c,y+ky-1,x+kx-1] -> (Co, Ci, 3, 3), in the dtype of the operands: the batch as the channels of a
    convolution of x with g as its (H x W) kernel"""
    return F.conv2d(x.transpose(0, 1), g.transpose(0, 1), None, 1, 1).transpose(0, 1).contiguous()


def flipped(w):
    """W'[c, o, ky, kx] = W[o, c, 2 - ky, 2 - kx]: grad_x = conv(g, W')"""
    return w.flip(2, 3).transpose(0, 1).contiguous()


Gradient = namedtuple("Gradient", "T S y32 g64 E32")
Reference = namedtuple("Reference", "x weight bias s")


def reference(x, w, g, has_bias=True):
    """x (B, Ci, H, W), w (Co, Ci, 3, 3), g = grad_y (B, Co, H, W), fp32 on the CPU -> Reference of Gradients (x: (B, Ci, H, W), weight:
    (Co, Ci, 3, 3), bias: (Co) or None)"""
    s = scale_of(g.abs().max().item())
    gs = g * s
    assert torch.equal((gs / s), g) or not torch.isfinite(g).all()       # (a power of two: exact)
    gh, gl = split(gs)
    xh, xl = split(x)
    wf = flipped(w)
    wh, wl = split(wf)
    d = torch.double
    # plain fp32 autograd on the CPU, and fp64 of the same
    leaves = [t.clone().requires_grad_() for t in (x, w)] + ([torch.zeros(w.size(0), requires_grad=True)] if has_bias else [])
    g32 = torch.autograd.grad(F.conv2d(leaves[0], leaves[1], leaves[2] if has_bias else None, 1, 1), leaves, g)
    g64x, g64w = F.conv2d(g.to(d), wf.to(d), None, 1, 1), wgrad(x.to(d), g.to(d))
    # weight
    Tw = (wgrad(xh.to(d) + xl.to(d), gh.to(d)) + wgrad(xh.to(d), gl.to(d))) / s
    Sw = wgrad(xh.abs().to(d), gh.abs().to(d)) / s
    yw = wgrad(torch.cat([xh, xl, xh]), torch.cat([gh, gh, gl])) / s
    weight = Gradient(Tw, Sw, yw, g64w, (g32[1].to(d) - g64w).abs().max().item())
    # input
    Tx = F.conv2d(torch.cat([gh, gl], 1).to(d), torch.cat([wh.to(d) + wl.to(d), wh.to(d)], 1), None, 1, 1) / s
    Sx = F.conv2d(gh.abs().to(d), wh.abs().to(d), None, 1, 1) / s
    yx = F.conv2d(torch.cat([gh, gh, gl], 1), torch.cat([wh, wl, wh], 1), None, 1, 1) / s
    gx = Gradient(Tx, Sx, yx, g64x, (g32[0].to(d) - g64x).abs().max().item())
    bias = None
    if has_bias:
        Tb = g.to(d).sum((0, 2, 3))
        bias = Gradient(Tb, g.to(d).abs().sum((0, 2, 3)), g.sum((0, 2, 3)), Tb, (g32[2].to(d) - Tb).abs().max().item())
    return Reference(gx, weight, bias, s)


def measure(y, r):
    """-> dict(r16, r32, err, bound): the two sides of assertion 1 and of assertion 2.  Elements with S = 0 (nothing to sum) must be
    exactly 0 and are left out of the ratios."""
    yd = y.detach().double().cpu()
    pos = r.S > 0
    assert not yd[~pos].any(), "an element with nothing to sum is not exactly 0"
    S = torch.where(pos, r.S, torch.ones_like(r.S))
    r16 = ((yd - r.T).abs() / S)[pos].max().item() if pos.any() else 0.0
    r32 = ((r.y32.double() - r.T).abs() / S)[pos].max().item() if pos.any() else 0.0
    return dict(r16=r16, r32=r32, err=(yd - r.g64).abs().max().item(), bound=4 * max(r.E32, 1e-6 * r.g64.abs().max().item()))


def check(what, y, r):
    """Both assertions on the gradient y against the Gradient r; prints error / bound first"""
    assert tuple(y.shape) == tuple(r.T.shape), (what, tuple(y.shape), tuple(r.T.shape))
    assert torch.isfinite(y).all(), f"{what}: not finite"
    m = measure(y, r)
    print(f"{what}: 1. |y - T| / S {m['r16']:.3e} <= {K16:.0f} * {m['r32']:.3e} (ratio {m['r16'] / m['r32'] if m['r32'] else float('nan'):.2f});  "
          f"2. |y - g64| {m['err']:.3e} <= {m['bound']:.3e} ({m['err'] / m['bound'] if m['bound'] else float('nan'):.3f} of the bound; "
          f"E32 {r.E32:.3e}, max |g64| {r.g64.abs().max().item():.3e})")
    assert m["r16"] <= K16 * m["r32"], (what, m)
    assert m["err"] <= m["bound"], (what, m)
    return m


# ---- the cases both test files use -----------------------------------------------------------------------------------------------------------
SHAPES = [(2, 32, 32, 64, 64), (3, 16, 48, 128, 64), (1, 32, 16, 64, 192)]      # (B, H, W, Ci, Co)
# the route cases (tests/test_train_routes_cpu.py asserts each reaches what it is there for, tests/test_train_routes_gpu.py runs them)
RouteCase = namedtuple("RouteCase", "id shape why")
ROUTE_CASES = [
    RouteCase("blocks_2x2", (1, 16, 16, 128, 128), "four channel blocks, two on each axis: blockIdx.y splits into (co block, ci block)"),
    RouteCase("blocks_3x2", (1, 16, 32, 128, 192), "six channel blocks, 3 x 2"),
    RouteCase("ragged_prep", (5, 48, 80, 64, 64), "pchunk = 75 (no multiple of 16), nprep = 256, 38 parts, the last of 4 tiles"),
    RouteCase("prep_scan_twice", (5, 48, 80, 64, 128), "nprep ncb = 512 > 256: the maximum scan of k_prep_finish goes round again"),
    RouteCase("chunk_9", (3, 208, 224, 64, 64), "chunk = 9, 243 parts, parts that straddle frames; pchunk = 546"),
]
OPERATOR_SHAPES = SHAPES + [(1, 32, 16, 64, 64)]      # every shape of the operator tests of tests/test_conv_bwd_gpu.py (the last: the halo's)


def inputs(B, H, W, Ci, Co, seed=0, g_scale=1.0):
    """x = relu(randn * 1.5), w, bias, g = g_scale * randn; deterministic, on the CPU"""
    gen = torch.Generator().manual_seed(1234 + seed + 7 * Ci + Co + H)
    x = torch.relu(torch.randn(B, Ci, H, W, generator=gen) * 1.5)
    w = torch.randn(Co, Ci, 3, 3, generator=gen) / (3 * Ci ** 0.5)
    b = torch.randn(Co, generator=gen)
    g = torch.randn(B, Co, H, W, generator=gen) * g_scale
    return x, w, b, g


def small_gradients(B, H, W, Ci, Co):
    """The first shape's inputs with g = 1e-7 * randn, one region a further 1e-3 smaller"""
    x, w, b, g = inputs(B, H, W, Ci, Co, seed=1, g_scale=1e-7)
    g[:, : Co // 2, : H // 2] *= 1e-3
    return x, w, b, g
