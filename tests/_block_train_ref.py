"""Shared by tests/test_block_train_cpu.py and tests/test_block_train_gpu.py (no tests in here): fp64 formulas of the three gradients of
csrc/block_train.hip through torch's own fp64 autograd, a pure-Python mirror of the split of the pixels into parts, and the bounds.

Bounds, with u = 2^-24 (the unit roundoff of fp32) and the fp64 result as the truth (its own error, 2^-53 per operation, is 2^-29 of u):

  The project's rule for a gradient:  |y - g64| <= 4 max(E32, 1e-6 max |g64|),  E32 = max |g32 - g64| of torch's own fp32 backward pass on the
  host -- a route is as good as another fp32 route of the same formula, with a floor for gradients fp32 gets exactly.

  Adjoints, per element:  |y - y64| <= 1.01 k u sum_i |w_i g_i|.  The kernel forms k terms w_i g_i, each ONE rounded product (w_i itself, a
  product of 0.25, 0.75 and 1, is exact), and adds them one after another: the sum of k terms rounds k - 1 times (the first add, to 0, is
  exact), and a partial sum never exceeds sum |w g| (1 + u)^k.  So every term's relative error is at most (1 + u)^k - 1 <= 1.01 k u for
  k <= 17.  "Down" sums its terms first (k' - 1 roundings for k' terms, weights 1) and multiplies once by 1.0f / 9.0f: that constant is
  1/9 (1 + d), |d| <= u, and the product rounds once more -- k' + 1 roundings, so k = k' + 1, and w_i = 1/9.  sum |w g| is the fp64
  adjoint applied to |g|: every weight is >= 0.

  grad_weight, per element:  |dW - dW64| <= 1.01 (L + parts) u sum_p |g[p][o]| |x[p][c]|.  v_mfma_f32_16x16x4_f32 is a chain of fp32
  fused multiply-adds: a wavefront that sees n pixels of a part rounds n times; the WAVES wavefronts of the part are added in order
  (WAVES - 1 roundings) and the parts likewise (parts - 1).  L = the largest n of any wavefront + WAVES is what chain() reports; a term
  passes through at most L + parts roundings, and (1 + u)^(L + parts) - 1 <= 1.01 (L + parts) u while (L + parts) u < 0.01: 160 000
  roundings, far beyond what the tests (and the decoder's 4096-pixel parts) reach.
"""
from collections import namedtuple

import torch
import torch.nn.functional as F

U = 2.0 ** -24
MAX_PARTS, MIN_PART, WAVES, MAX_CHANNELS = 256, 512, 8, 256

UP_SHAPES = [(1, 1, 3, 4), (2, 2, 2, 8), (1, 5, 4, 64)]          # (B, H, W, C) of grad_in
DOWN_SHAPES = [(1, 2, 2, 4), (2, 4, 6, 8), (1, 6, 16, 64)]
GW_SHAPES = [(16, 64, 64), (3 * 6 * 8, 64, 128), (2 * 16 * 16, 256, 128), (1040, 128, 256)]       # (npix, Ci, Co)


# ---- the split of the pixels (include/pixelsynth_block_train.h) ---------------------------------------------------------------------------
def sizes_ok(npix, Ci, Co):
    return npix > 0 and npix % 16 == 0 and Ci > 0 and Co > 0 and Ci % 16 == 0 and Co % 16 == 0 and Ci <= MAX_CHANNELS and Co <= MAX_CHANNELS


def tiles(Ci, Co):
    """-> (chunks of g a workgroup takes, chunks of x, number of workgroups per part)"""
    nbo, nbc = -(-Co // 64), -(-Ci // 64)
    TO = 2 if nbo % 2 == 0 else 1
    TC = 2 if TO == 1 and nbc % 2 == 0 else 1
    return TO, TC, (nbo // TO) * (nbc // TC)


def part_ranges(npix, Ci, Co):
    """[(first pixel, one past the last)] of every part, in order; [] for sizes the library refuses"""
    if not sizes_ok(npix, Ci, Co):
        return []
    target = min(MAX_PARTS, max(1, 512 // tiles(Ci, Co)[2]))
    part = max(MIN_PART, 16 * -(-(npix // 16) // target))
    return [(p, min(npix, p + part)) for p in range(0, npix, part)]


def wave_pixels(lo, hi):
    """The pixels wavefront w of a part [lo, hi) accumulates, in its order: the groups of four w, w + WAVES, ..."""
    return [[p + k for p in range(lo + 4 * w, hi, 4 * WAVES) for k in range(4)] for w in range(WAVES)]


def chain(npix, Ci, Co):
    """L of the docstring: the most pixels any wavefront accumulates, plus the wavefronts added after it"""
    return max(len(w) for lo, hi in part_ranges(npix, Ci, Co) for w in wave_pixels(lo, hi)) + WAVES


GwPlan = namedtuple("GwPlan", "TO TC tiles_o tiles_c short_g short_x part_pix parts last_pix")


def gw_plan(npix, Ci, Co):
    """gw_plan of csrc/block_train.hip: the kernel is k_grad_weight<TO, TC> on a tiles_o x tiles_c grid of workgroups per part; short_g /
    short_x: the channels of the last 64-channel chunk of g / x when it ends early (on_g / on_x false for the lanes past them), else 0;
    pixels of a part, parts, pixels of the last part"""
    TO, TC, _ = tiles(Ci, Co)
    parts = part_ranges(npix, Ci, Co)
    return GwPlan(TO, TC, -(-Co // 64) // TO, -(-Ci // 64) // TC, Co % 64, Ci % 64, parts[0][1] - parts[0][0], len(parts),
                  parts[-1][1] - parts[-1][0])


# ---- the route cases (tests/test_train_routes_cpu.py asserts each reaches what it is there for, tests/test_train_routes_gpu.py runs them) --
GW_ROUTE_SHAPES = [(528, 128, 64), (528, 80, 48), (528, 48, 80), (528, 192, 192), (528, 256, 192), (131088, 16, 16)]     # (npix, Ci, Co)
BIG_RESAMPLE = (2, 258, 256, 64)                    # (B, H, W, C) of grad_in: 2^21 + 16 384 float4s, 8192 workgroups of 256 take 2^21 at a time
UP_ROUTE_SHAPES = [(1, 3, 1, 4), BIG_RESAMPLE]
DOWN_ROUTE_SHAPES = [BIG_RESAMPLE]
GRID_MAX, GRID_THREADS = 256 * 32, 256              # grid_for of csrc/block_train.hip


def second_trip(shape4):
    """(float4s of grad_in, those a thread reaches only on its second trip of the grid-stride loop, the rows of the last frame they are
    -- None unless they are whole rows of the last frame)"""
    B, H, W, C = shape4
    total4, first = B * H * W * C // 4, GRID_MAX * GRID_THREADS
    rest = max(0, total4 - first)
    row4 = W * C // 4
    rows = rest // row4 if rest % row4 == 0 and rest <= H * row4 else None
    return total4, rest, rows


# ---- fp64 formulas: torch's own autograd in fp64 on the host ------------------------------------------------------------------------------------
def resample(kind, x):
    if kind == "Up":
        return F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
    return F.avg_pool2d(x, kernel_size=3, stride=2, padding=1)


def adjoint(kind, g, shape, dtype=torch.float64):
    """R^T g for R = resample(kind, .) on inputs of `shape` (B, C, H, W): autograd of <R(a), g> in `dtype`"""
    a = torch.zeros(shape, dtype=dtype, requires_grad=True)
    (resample(kind, a) * g.to(dtype)).sum().backward()
    return a.grad


def axis_terms(kind, n):
    """Per index i of an axis of n inputs, the number of outputs it hears from with a weight that is not 0 (the header's tables): "Up"
    2 i - 1 (i >= 1), 2 i, 2 i + 1, 2 i + 2 (i <= n - 2); "Down" i / 2 and, for an odd i, (i + 1) / 2 where that is an output"""
    i = torch.arange(n)
    if kind == "Up":
        return ((i >= 1).double() + 2 + (i <= n - 2).double())
    return 1 + ((i % 2 == 1) & ((i + 1) // 2 < n // 2)).double()


def adjoint_terms(kind, shape):
    """k of the docstring per element of grad_in (B, C, H, W): the number of outputs the pixel hears from with a weight that is not 0,
    plus 1 for "Down".  Both resamplings are separable, so it is the product of the two axes' counts (tests/test_train_routes_cpu.py
    holds it equal to adjoint_terms_loop at UP_SHAPES and DOWN_SHAPES)"""
    B, C, H, W = shape
    count = axis_terms(kind, H).view(H, 1) * axis_terms(kind, W).view(1, W)
    return (count + (kind == "Down")).view(1, 1, H, W).expand(shape)


def adjoint_terms_loop(kind, shape):
    """adjoint_terms by one autograd call per output pixel: what the closed form is held to at the small shapes"""
    n = adjoint(kind, torch.ones(resample(kind, torch.zeros(shape, dtype=torch.float64)).shape), shape)      # the weights' sum: only to be sure
    assert (n > 0).all()
    B, C, H, W = shape
    out = resample(kind, torch.zeros(1, 1, H, W, dtype=torch.float64)).shape[2:]
    count = torch.zeros(H, W, dtype=torch.float64)
    for Y in range(out[0]):
        for X in range(out[1]):
            g = torch.zeros(1, 1, *out, dtype=torch.float64)
            g[0, 0, Y, X] = 1.0
            count += (adjoint(kind, g, (1, 1, H, W))[0, 0] != 0).double()
    return (count + (kind == "Down")).view(1, 1, H, W).expand(shape)


def adjoint_bound(kind, g, shape):
    return 1.01 * adjoint_terms(kind, shape) * U * adjoint(kind, g.abs(), shape)


def conv1x1_grads(x, w, b, g, dtype=torch.float64):
    """(grad_input, grad_weight, grad_bias) of <conv2d(x, w, b), g> by autograd in `dtype`; x (B, Ci, H, W), w (Co, Ci, 1, 1), b (Co)"""
    x, w, b = (t.detach().to(dtype).clone().requires_grad_() for t in (x, w, b))
    (F.conv2d(x, w, b) * g.to(dtype)).sum().backward()
    return x.grad, w.grad, b.grad


def grad_weight_bound(x, g, npix, Ci, Co):
    """1.01 (L + parts) u sum_p |g[p][o]| |x[p][c]| as (Co, Ci, 1, 1)"""
    ga, xa = g.double().abs().permute(1, 0, 2, 3).reshape(Co, -1), x.double().abs().permute(1, 0, 2, 3).reshape(Ci, -1)
    return (1.01 * (chain(npix, Ci, Co) + len(part_ranges(npix, Ci, Co))) * U * (ga @ xa.t())).view(Co, Ci, 1, 1)


def grad_bound(g32, g64):
    """The project's rule -> (bound, E32)"""
    E32 = (g32.double() - g64).abs().max().item()
    return 4 * max(E32, 1e-6 * g64.abs().max().item()), E32


def check(name, got, want, bound):
    """max |got - want| / bound, printed and returned; bound a number or a tensor of want's shape.  A bound of 0 asks for got == want."""
    assert got.shape == want.shape and torch.isfinite(got).all(), name
    err = (got.double().cpu() - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: max |err| {err.max().item():.3e}, error / bound {ratio:.3f}")
    return ratio


def gw_inputs(npix, Ci, Co, seed=0):
    """x (B, Ci, H, W), w (Co, Ci, 1, 1), b (Co), g (B, Co, H, W) with B H W = npix"""
    B, H, W = {16: (1, 4, 4), 144: (3, 6, 8), 512: (2, 16, 16), 1040: (1, 26, 40)}.get(npix, (1, npix // 16, 16))
    assert B * H * W == npix
    gen = torch.Generator().manual_seed(seed + npix + Ci)
    return (torch.randn(B, Ci, H, W, generator=gen), torch.randn(Co, Ci, 1, 1, generator=gen) * Ci ** -0.5, torch.randn(Co, generator=gen),
            torch.randn(B, Co, H, W, generator=gen))
