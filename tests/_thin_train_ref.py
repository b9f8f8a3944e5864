"""Shared by tests/test_thin_train_cpu.py and tests/test_thin_train_gpu.py (no tests in here): fp64 formulas of the three gradients of a thin
convolution through torch's own fp64 autograd, a pure-Python restatement of the split of the pixels into parts and groups
(include/pixelsynth_thin_train.h), and the bounds.

Bounds, with u = 2^-24 (the unit roundoff of fp32) and the fp64 result as the truth (its own error, 2^-53 per operation, is 2^-29 of u):

  The project's rule for a gradient:  |y - g64| <= 4 max(E32, 1e-6 max |g64|),  E32 = max |g32 - g64| of torch's own fp32 backward pass of
  the same formula on the host -- a route is as good as another fp32 route, with a floor for gradients fp32 gets exactly.

  ps_thin_expand_f32, per element:  |y - y64| <= 1.01 n u sum |w g|,  n the number of summed terms: T per tap inside the frame.  The sum
  starts at 0 and takes one fused multiply-add per term -- n roundings, none for the product -- and a partial sum never exceeds
  sum |w g| (1 + u)^n, so every term's relative error is at most (1 + u)^n - 1 <= 1.01 n u (n <= 36).  sum |w g| is the fp64 formula on
  |w| and |g|.

  grad_weight, per element:  |dW - dW64| <= 1.01 (L + parts) u sum_p |thin| |wide|.  A group of a part takes n of its pixels in one chain of
  fused multiply-adds (n roundings), the GROUPS groups are added in ascending order (GROUPS - 1 roundings) and the parts likewise
  (parts - 1).  L = the largest n of any group + GROUPS is what chain() reports; a term passes through at most L + parts roundings, and
  (1 + u)^(L + parts) - 1 <= 1.01 (L + parts) u while (L + parts) u < 0.01.  grad_bias takes the same walk in fp64 and is rounded to fp32
  once, so it is held to the same rule with sum_p |g| and meets it with room to spare: its error is u |grad_bias| and fp64's own.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
MAX_PARTS, MIN_PART, GROUPS, MAX_WIDE = 256, 1024, 32, 256

FRAMES = [(1, 8, 64), (2, 16, 64), (3, 8, 128)]         # (B, H, W)
WIDE = [32, 64, 128]
THIN_OUT = [1, 3, 4]
KS = [1, 3]
RAGGED = (5, 8, 64)                                      # 2560 pixels: parts of 1024, 1024 and 512
DECODER_LAYERS = [("in", 4, 64, 3), ("in", 4, 64, 1), ("out", 128, 3, 3), ("out", 128, 3, 1)]          # (kind, Ci, Co, k) at 256 x 256


# ---- the split of the pixels (include/pixelsynth_thin_train.h) ----------------------------------------------------------------------------
def sizes_ok(B, H, W, Cw, T, k):
    return (B > 0 and H > 0 and W > 0 and B * H * W < 2 ** 31 and Cw > 0 and Cw % 32 == 0 and Cw <= MAX_WIDE and 1 <= T <= 4
            and k in (1, 3))


def part_ranges(npix):
    """[(first pixel, one past the last)] of every part, in order"""
    part = max(MIN_PART, GROUPS * -(-(-(-npix // GROUPS)) // MAX_PARTS))
    return [(p, min(npix, p + part)) for p in range(0, npix, part)]


def group_pixels(lo, hi):
    """The pixels group q of a part [lo, hi) accumulates, in its order: lo + q, lo + q + GROUPS, ..."""
    return [list(range(lo + q, hi, GROUPS)) for q in range(GROUPS)]


def chain(npix):
    """L of the docstring: the most pixels any group accumulates, plus the groups added after it"""
    return max(-(-(hi - lo) // GROUPS) for lo, hi in part_ranges(npix)) + GROUPS


def workspace_bytes(B, H, W, Cw, T, k):
    return -(-(len(part_ranges(B * H * W)) * (k * k * T * Cw + 2 * Cw) * 4) // 256) * 256


# ---- fp64 formulas: torch's own autograd on the host --------------------------------------------------------------------------------------
def conv_grads(x, w, b, g, dtype=torch.float64):
    """(grad_input, grad_weight, grad_bias) of <conv2d(x, w, b, padding = k / 2), g> by autograd in `dtype`"""
    x, w, b = (t.detach().to(dtype).clone().requires_grad_() for t in (x, w, b))
    (F.conv2d(x, w, b, padding=w.size(2) // 2) * g.to(dtype)).sum().backward()
    return x.grad, w.grad, b.grad


def abs_grads(x, w, g):
    """The three formulas on absolute values: sum |w| |g| per input element, sum |g| |x| per weight, sum |g| per bias"""
    return conv_grads(x.abs(), w.abs(), torch.zeros(w.size(0)), g.abs())


def expand_terms(shape, T, k):
    """n of the docstring per element of grad_input (B, Cw, H, W): T per tap that lies inside the frame"""
    B, Cw, H, W = shape
    one = torch.ones(1, 1, H, W, dtype=torch.float64)
    taps = F.conv2d(one, torch.ones(1, 1, k, k, dtype=torch.float64), padding=k // 2)
    return (T * taps).expand(shape)


def expand_bound(x, w, g):
    return 1.01 * expand_terms(x.shape, w.size(0), w.size(2)) * U * abs_grads(x, w, g)[0]


def sums_bound(x, w, g):
    """(bound of grad_weight, bound of grad_bias): 1.01 (L + parts) u times the sums of absolute values"""
    npix = x.size(0) * x.size(2) * x.size(3)
    _, aw, ab = abs_grads(x, w, g)
    f = 1.01 * (chain(npix) + len(part_ranges(npix))) * U
    return f * aw, f * ab


def grad_bound(g32, g64, floor=None):
    """The project's rule -> (bound, E32); `floor`: another error to hold the route to in place of E32"""
    E32 = (g32.double() - g64).abs().max().item() if floor is None else floor
    return 4 * max(E32, 1e-6 * g64.abs().max().item()), E32


def check(name, got, want, bound):
    """max |got - want| / bound, printed and returned; bound a number or a tensor of want's shape.  A bound of 0 asks for got == want."""
    assert got.shape == want.shape and torch.isfinite(got).all(), name
    err = (got.double().cpu() - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ratio = torch.where(err == 0, torch.zeros_like(err), err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: max |err| {err.max().item():.3e}, error / bound {ratio:.3f}")
    return ratio


def inputs(kind, frame, wide, T, k, seed=0):
    """x (B, Ci, H, W), w (Co, Ci, k, k), b (Co), g (B, Co, H, W) of a thin-in (4 -> wide) or thin-out (wide -> T) layer"""
    B, H, W = frame
    Ci, Co = (4, wide) if kind == "in" else (wide, T)
    gen = torch.Generator().manual_seed(seed + 7 * B + H + W + wide + 13 * T + k)
    return (torch.randn(B, Ci, H, W, generator=gen), torch.randn(Co, Ci, k, k, generator=gen) * (Ci * k * k) ** -0.5,
            torch.randn(Co, generator=gen), torch.randn(B, Co, H, W, generator=gen))
