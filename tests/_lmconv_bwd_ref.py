"""The fp64 side of the tests of the locally masked convolution's backward pass (csrc/lmconv_bwd.hip): the expected gradients, the
adjoint mask, and the rounding bounds.  Not a test module.

Expected values: torch autograd in fp64 through oracle.lmconv_oracle.lmconv (the reference's unfold formula) on the SAME fp32 inputs.

THE BOUNDS are derived, not measured.  With u = 2^-24 (half an ulp, relative), B*L locations, and PARTS = 64 the most partial results a
sum is split into (PS_LMCONV_BWD_MAX_PARTS of include/pixelsynth_lmconv_bwd.h):

    |d grad_W[o,c,t]| <= 1.01 (B L + 66) u sum_{b,l} |g| |m| |xpad|
    |d grad_bias[o]|  <= 1.01 (B L + 66) u sum_{b,l} |g|
    |d grad_x[b,c,p]| <= 1.01 (9 Co + 66) u sum_{t,o} |W| |m| |g|

A sum of n products accumulated by fused multiply-adds, in whatever order and split into however many chains, rounds once per
accumulation: every term passes at most n roundings, (1 + u)^n - 1 <= 1.01 n u for n u < 0.01.  The 66 = PARTS + 2 pays for at most 64
additions of partial sums and for the product of the mask value with the shifted input (one rounding, before the chain), with one to
spare.  Where a bound is 0 -- every tap closed, or outside the grid -- the result must be exactly 0.

The forward's own bound is stated at forward64().  plan() mirrors the kernel's split of the reduction; ROUTE_CASES are the shapes that take
the steps, parts and location walks the operator shapes (OPERATOR_SHAPES) leave out.
"""
from collections import namedtuple

import torch

from oracle import lmconv_oracle as lo

U = 2.0 ** -24
MAX_PARTS = 64                     # = PS_LMCONV_BWD_MAX_PARTS (test_lmconv_bwd_cpu.py reads the header)
SLACK = MAX_PARTS + 2


TILE, BLOCK, KSTEP, DEPTH, TARGET_WAVES = 16, 32, 4, 4, 256 * 4 * 4      # csrc/lmconv_bwd.hip's
LmPlan = namedtuple("LmPlan", "N ksteps chunk parts last bytes")


def plan(B, Ci, Co, H, W):
    """csrc/lmconv_bwd.hip's make_plan: locations, steps of KSTEP locations, steps per part, parts, the last part's steps, and the
    workspace's size (which tests/test_train_routes2_cpu.py holds to the library's own: it fixes parts)"""
    up = lambda v: -(-v // 256) * 256
    N = B * H * W
    Cop, Cip = -(-Co // TILE) * TILE, -(-Ci // TILE) * TILE
    ksteps, tasks = -(-N // KSTEP), 9 * -(-Cop // BLOCK) * -(-Cip // BLOCK)
    want = max(1, min(-(-TARGET_WAVES // tasks), MAX_PARTS, ksteps))
    chunk = -(-ksteps // want)
    parts = -(-ksteps // chunk)
    return LmPlan(N, ksteps, chunk, parts, ksteps - (parts - 1) * chunk, up(up(up(N * Cop * 4) + N * Cip * 4) + parts * 9 * Cop * Cip * 4))


RouteCase = namedtuple("RouteCase", "id shape why")          # shape (B, Ci, Co, H, W, dilation)
ROUTE_CASES = [
    RouteCase("chunk6_short_last", (2, 16, 16, 15, 43, 1), "chunk = 6: the second batch of a part holds two steps; 54 parts, the last of 5 steps; N % 4 = 2"),
    RouteCase("chunk6_d2", (1, 16, 16, 37, 35, 2), "chunk = 6 at dilation 2; N % 4 = 3"),
    RouteCase("chunk3", (4, 160, 80, 8, 8, 1), "chunk = 3: a batch with one step closed in every part; 22 parts, the last of 1 step"),
    RouteCase("grid_1x1", (5, 3, 2, 1, 1, 1), "five locations: a lane's step of 4 crosses four images, both whiles loop"),
    RouteCase("grid_2x1_d2", (3, 3, 2, 2, 1, 2), "W = 1, and every off-centre tap closed by the dilation"),
    RouteCase("grid_3x3", (2, 5, 3, 3, 3, 1), "W = 3 < KSTEP: a step always changes the row"),
    RouteCase("row_1x3", (7, 20, 40, 1, 3, 1), "H = 1: a step always changes the image; Co = 40: two tiles of 16 in one block, the second short"),
    RouteCase("dilation_past_grid", (2, 7, 5, 6, 9, 7), "dilation 7 >= H = 6: every off-centre row closed, the columns open at the rims"),
]
# (B, Ci, Co, H, W, dilation) of the operator and network tests of tests/test_lmconv_bwd_gpu.py
OPERATOR_SHAPES = [(3, 7, 5, 6, 9, 2), (2, 7, 5, 6, 9, 1), (2, 7, 5, 6, 9, 2), (2, 160, 80, 8, 8, 1), (2, 160, 160, 8, 8, 1), (2, 80, 80, 8, 8, 2),
                   (2, 80, 80, 8, 8, 1), (1, 513, 80, 8, 8, 1), (2, 513, 80, 8, 8, 1), (5, 16, 16, 32, 32, 1)]


def inputs(B, Ci, Co, H, W, seed):
    """Per-image fractional masks with zeros throughout, as tests/test_lmconv_bwd_gpu.py's _inputs(..., frac=True) makes them (the same
    draws in the same order).  On a grid of fewer than ten locations the centre tap of image 0 is opened: five 1 x 1 images have all
    five centre taps closed once in a hundred seeds, and every gradient but the bias's is then an exact 0 that proves nothing."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, Ci, H, W, generator=gen)
    w = torch.randn(Co, Ci, 3, 3, generator=gen) * 0.1
    b = torch.randn(Co, generator=gen)
    m = torch.rand(B, 9, H * W, generator=gen)
    m = torch.where(m < 0.4, torch.zeros_like(m), m)
    g = torch.randn(B, Co, H, W, generator=gen)
    if H * W < 10:
        m[0, 4] = 0.75
    return x, m, w, b, g


def forward64(x, m, w, bias, dilation):
    """-> (y in fp64 by the oracle's unfold formula on the same fp32 inputs, its bound):

        |d y[b,o,l]| <= 1.01 (9 Ci + 2) u (|bias[o]| + sum_{c,t} |W| |m| |xpad|)

    y is a sum of 9 Ci + 1 terms, the bias among them.  Added in whatever order and split into however many chains (the forward kernel
    keeps one set of accumulators per tap, adds the taps of a row, then the three rows and the bias), a term passes at most 9 Ci
    additions that round -- one that adds an exact 0, a closed tap or a padded channel, does not -- and a fused multiply-add's product
    does not round on its own; the product of the mask value with the shifted input rounds once before the chain: 9 Ci + 1, with one
    to spare as in the gradients' bounds.  Where the bound is 0 -- every tap closed and no bias -- y must be exactly 0."""
    x, m, w, bias = (None if t is None else t.detach().cpu().double() for t in (x, m, w, bias))
    y = lo.lmconv(x, m, w, bias, dilation)
    mag = lo.lmconv(x.abs(), m.abs(), w.abs(), None if bias is None else bias.abs(), dilation)
    return y, 1.01 * (9 * x.shape[1] + 2) * U * mag


def adjoint_mask(m, H, W, dilation):
    """m (Bm,9,L) -> m'[b,t,p] = m[b,8-t,p+off(t)] where p+off(t) lies in the grid, 0 elsewhere"""
    Bm = m.shape[0]
    src = m.reshape(Bm, 9, H, W)
    out = torch.zeros_like(src)
    for t in range(9):
        di, dj = (t // 3 - 1) * dilation, (t % 3 - 1) * dilation
        i0, i1, j0, j1 = max(0, -di), min(H, H - di), max(0, -dj), min(W, W - dj)
        if i0 < i1 and j0 < j1:
            out[:, t, i0:i1, j0:j1] = src[:, 8 - t, i0 + di:i1 + di, j0 + dj:j1 + dj]
    return out.reshape(Bm, 9, H * W)


def adjoint_weight(w):
    """W'[c,o,t] = W[o,c,8-t]"""
    return w.flip(2, 3).transpose(0, 1).contiguous()


def gradients(x, m, w, bias, g, dilation, dtype=torch.float64):
    """torch autograd through the oracle's lmconv at `dtype` on CPU copies -> (grad_x, grad_w, grad_bias or None)"""
    x, w, g = (t.detach().cpu().to(dtype) for t in (x, w, g))
    m = m.detach().cpu().to(dtype)
    x.requires_grad_()
    w.requires_grad_()
    b = None if bias is None else bias.detach().cpu().to(dtype).requires_grad_()
    y = lo.lmconv(x, m, w, b, dilation)
    return torch.autograd.grad(y, (x, w) if b is None else (x, w, b), g) + ((None,) if b is None else ())


def bounds(x, m, w, g, dilation):
    """-> (bound of grad_x, of grad_w, of grad_bias), fp64: the formulas of this module's docstring"""
    B, _, H, W = x.shape
    Co = w.shape[0]
    ax, aw, _ = gradients(x.abs(), m.abs(), w.abs(), None, g.abs(), dilation)
    ab = g.detach().cpu().double().abs().sum((0, 2, 3))
    n = B * H * W
    return 1.01 * (9 * Co + SLACK) * U * ax, 1.01 * (n + SLACK) * U * aw, 1.01 * (n + SLACK) * U * ab


def ratio(got, want, bound):
    """The largest |got - want| / bound over the entries with a bound; where the bound is 0, got must be exactly 0 (AssertionError)"""
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape == bound.shape, (got.shape, want.shape, bound.shape)
    assert torch.isfinite(got).all()
    closed = bound == 0
    assert (got[closed] == 0).all(), "a result whose every term is closed must be exactly 0"
    if closed.all():
        return 0.0
    return float(((got - want).abs()[~closed] / bound[~closed]).max())


def check(name, got, want, bound):
    r = ratio(got, want, bound)
    print(f"{name}: largest error / bound {r:.4f}")
    assert r <= 1.0, (name, r)
    return r
