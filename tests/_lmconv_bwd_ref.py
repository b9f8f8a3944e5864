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
"""
import torch

from oracle import lmconv_oracle as lo

U = 2.0 ** -24
MAX_PARTS = 64                     # = PS_LMCONV_BWD_MAX_PARTS (test_lmconv_bwd_cpu.py reads the header)
SLACK = MAX_PARTS + 2


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
