"""Shared by tests/test_thin_train_cpu.py, tests/test_thin_train_gpu.py, tests/test_thin_routes_cpu.py and tests/test_thin_routes_gpu.py (no
tests in here): fp64 formulas of the three gradients of a thin convolution through torch's own fp64 autograd, a pure-Python restatement of
the split of the pixels into parts and groups (include/pixelsynth_thin_train.h), the bounds, and -- for the route tests -- one predicate
per branch of csrc/thin_train.hip that the first tables (FRAMES, RAGGED, WIDE, THIN_OUT) never take, with ROUTES and BIAS_ROUTES, the
named cases that take them.

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


def layer_inputs(Ci, Co, frame, k, seed=0):
    """x (B, Ci, H, W), w (Co, Ci, k, k), b (Co), g (B, Co, H, W) of any convolution: the layers the entry points take and the Functions
    refuse (a thin side of 1 .. 3 channels on the way in, frames of any height and width)"""
    B, H, W = frame
    gen = torch.Generator().manual_seed(seed + 7 * B + H + 3 * W + 5 * Ci + 13 * Co + k)
    return (torch.randn(B, Ci, H, W, generator=gen), torch.randn(Co, Ci, k, k, generator=gen) * (Ci * k * k) ** -0.5,
            torch.randn(Co, generator=gen), torch.randn(B, Co, H, W, generator=gen))


# ---- which branch a shape takes: csrc/thin_train.hip restated, one predicate per branch ---------------------------------------------------
THREADS, EX_ROWS, EX_PX, BIAS_GRID = 256, 8, 4, 256 * 32      # the unit's THREADS, EX_ROWS, EX_PX and grid_for()'s cap on the workgroups


def capped(npix):
    """gw_plan: part_pix = max(MIN_PART, GW_GROUPS * ceil(steps / MAX_PARTS)) takes its second operand -- parts longer than MIN_PART"""
    lo, hi = part_ranges(npix)[0]
    return hi - lo > MIN_PART


def sum_tail(npix):
    """k_thin_sum_parts: `for (p = 1; p < parts; ++p)` under #pragma unroll 32 runs an unrolled body (32 or more trips) and then a
    remainder"""
    trips = len(part_ranges(npix)) - 1
    return trips >= 32 and trips % 32 != 0


def walk(W):
    """k_thin_grad_weight: `xstep = GW_GROUPS % W, ystep = GW_GROUPS / W` -> (xstep, ystep)"""
    return GROUPS % W, GROUPS // W


def carry_period(W):
    """k_thin_grad_weight: `if (x >= W) { x -= W; ++y; }` -- the number of steps after which x is where it started (the carry's pattern
    repeats), None where x never moves"""
    xstep = walk(W)[0]
    return None if xstep == 0 else W // _gcd(W, xstep)


def _gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def second_step(npix):
    """k_thin_grad_weight: `for (; p < hi; p += GW_GROUPS)` runs twice for some group -- only then is the advanced (x, y) ever used"""
    return any(hi - lo > GROUPS for lo, hi in part_ranges(npix))


def double_wrap(H, W, npix=None):
    """k_thin_grad_weight: `if (y >= H) y %= H` -- a step (ystep rows and, where x + xstep passes W, a carry) leaves y at 2 H or beyond,
    where one subtraction of H is not the remainder.  With npix: a step that some thread of the batch takes and goes on from (its next pixel
    is inside its part); without: whether a frame of this height and width admits one at all"""
    xstep, ystep = walk(W)
    if H - 1 + ystep + (1 if xstep else 0) < 2 * H:
        return False
    if npix is None:
        return True
    return any((p // W) % H + ystep + (p % W + xstep >= W) >= 2 * H for lo, hi in part_ranges(npix) for p in range(lo, hi - GROUPS))


def empty_groups(npix):
    """k_thin_grad_weight: `size_t p = lo + grp; for (; p < hi; ...)` -- a part of fewer than GW_GROUPS pixels: a group whose loop never
    runs"""
    return any(hi - lo < GROUPS for lo, hi in part_ranges(npix))


def all_border(H, W, k=3):
    """k_thin_grad_weight: `if (y >= R && y + R < H && x >= R && x + R < W)` is true for no pixel of the frame"""
    return k == 3 and (H < 3 or W < 3)


def expand_workgroups(B, H):
    """k_thin_expand: `for (row = blockIdx.x * EX_ROWS; row < min(rows, (blockIdx.x + 1) * EX_ROWS); ++row)` -> [(first row, one past)]"""
    return [(r, min(B * H, r + EX_ROWS)) for r in range(0, B * H, EX_ROWS)]


def expand_straddles(B, H):
    """k_thin_expand: a workgroup's rows lie in two frames (`y = row % H` falls back to 0 inside its loop)"""
    return any(lo // H != (hi - 1) // H for lo, hi in expand_workgroups(B, H))


def expand_short_tail(B, H):
    """k_thin_expand: the min() of the last workgroup's loop takes `rows`"""
    return (B * H) % EX_ROWS != 0


def expand_mod_is_no_mask(H):
    """k_thin_expand: `y = row % H` differs from row & (H - 1)"""
    return H & (H - 1) != 0


def expand_one_window(W):
    """k_thin_expand: `on[i] = xx >= 0 && xx < W` over the NX = EX_PX + 2 pixels x0 - 1 .. x0 + 4 of one thread is false at both ends"""
    return W == EX_PX


def no_power_of_two(Cw):
    """`item % C4`, `item / C4` (k_thin_expand), `bias[i % C4]` (k_thin_add_bias4) with a C4 that is no shift and mask"""
    return Cw & (Cw - 1) != 0


def bias_route(npix, C, aligned):
    """ps_thin_add_bias_f32: `if (C % 4 == 0 && aligned16(y) && aligned16(bias))` -> (the kernel's elements per pixel, its elements)"""
    per = C // 4 if C % 4 == 0 and aligned else C
    return per, npix * per


def bias_loops(npix, C, aligned):
    """k_thin_add_bias4 / k_thin_add_bias1: `i += gridDim.x * THREADS` brings a thread to a second element (grid_for caps the grid)"""
    return bias_route(npix, C, aligned)[1] > BIAS_GRID * THREADS


def bias_stride_turns(npix, C, aligned):
    """... and that element has another channel than the first: the stride is no multiple of the pixel's elements"""
    return bias_loops(npix, C, aligned) and (BIAS_GRID * THREADS) % bias_route(npix, C, aligned)[0] != 0


def bias_scalar_c4(npix, C, aligned):
    """ps_thin_add_bias_f32: a C that is a multiple of 4 on the scalar kernel (y or bias not aligned to 16 bytes)"""
    return C % 4 == 0 and not aligned


def bias_partial_block(npix, C, aligned):
    """k_thin_add_bias4 / k_thin_add_bias1: `i < total` is false for a thread of the last workgroup"""
    return bias_route(npix, C, aligned)[1] % THREADS != 0


# ---- the routes no shape above takes ------------------------------------------------------------------------------------------------------
class Route:
    """A named case.  via: "function" (conv_thin_in_train / conv_thin_out_train, kind "in" / "out"), "grad_weight" or "expand" (the
    entry point itself, for shapes the Functions refuse; kind "in": wide_is_g = 1, "out": 0 -- "both": each in turn).  reaches: names of
    BRANCHES"""

    def __init__(self, id, via, kind, frame, wide, T, k, reaches):
        self.id, self.via, self.kind, self.frame, self.wide, self.T, self.k, self.reaches = id, via, kind, frame, wide, T, k, tuple(reaches)
        self.npix = frame[0] * frame[1] * frame[2]

    def __repr__(self):
        return self.id


def _gw(f):      # a branch of ps_thin_grad_weight_f32: every route but the expansion alone reaches that entry point
    return lambda r: r.via != "expand" and f(r)


def _ex(f):      # a branch of ps_thin_expand_f32: the thin-out Function's grad_input, or the entry point itself
    return lambda r: (r.via == "expand" or (r.via == "function" and r.kind == "out")) and f(r)


BRANCHES = {
    "capped": _gw(lambda r: capped(r.npix)),
    "sum-tail": _gw(lambda r: sum_tail(r.npix)),
    # (the walk: at k = 1 no tap looks at (x, y), and a thread that takes one pixel never advances them)
    "ystep": _gw(lambda r: r.k == 3 and walk(r.frame[2])[1] > 0 and second_step(r.npix)),
    "carry-period": _gw(lambda r: r.k == 3 and carry_period(r.frame[2]) not in (None, 1, 2, 4, 8, 16, 32) and second_step(r.npix)),
    "double-wrap": _gw(lambda r: r.k == 3 and double_wrap(r.frame[1], r.frame[2], r.npix)),
    "empty-groups": _gw(lambda r: empty_groups(r.npix)),
    "all-border": _gw(lambda r: all_border(r.frame[1], r.frame[2], r.k)),
    "straddle": _ex(lambda r: expand_straddles(r.frame[0], r.frame[1])),
    "short-tail": _ex(lambda r: expand_short_tail(r.frame[0], r.frame[1])),
    "row-mod": _ex(lambda r: expand_mod_is_no_mask(r.frame[1])),
    "one-window": _ex(lambda r: expand_one_window(r.frame[2])),
    "t2": lambda r: r.T == 2,
    "wide-max": lambda r: r.wide == MAX_WIDE,
    "wide-odd": lambda r: no_power_of_two(r.wide),
}


def _abi(via, frames, reaches):
    """Entry-point cases: every T in 1 .. 4 and k in {1, 3} on each frame (the GPU test loops over them; T = 2, k = 3 stands for all here)"""
    return [Route(f"{via}-{'x'.join(map(str, f))}", via, "both" if via == "grad_weight" else "out", f, 32, 2, 3, reaches[f]) for f in frames]


ROUTES = [
    # through the Functions (takes_in / takes_out sizes)
    Route("capped-ragged", "function", "out", (1, 520, 512), 32, 3, 3, ("capped", "sum-tail", "row-mod")),       # parts of 1056, 253 of them, the last of 128
    Route("capped-full-in", "function", "in", (5, 256, 256), 64, 4, 3, ("capped", "sum-tail")),       # 256 parts of 1280: the decoder's frame
    Route("capped-full-out", "function", "out", (5, 256, 256), 32, 4, 1, ("capped", "sum-tail")),
    Route("w32", "function", "out", (3, 8, 32), 32, 3, 3, ("ystep",)),                                # the walk (0, 1)
    Route("w96-t2", "function", "out", (2, 24, 96), 32, 2, 3, ("carry-period", "row-mod", "t2")),     # a carry every third step; 5 parts
    Route("w96-t4", "function", "out", (2, 24, 96), 32, 4, 3, ("carry-period", "row-mod")),
    Route("t2-k1", "function", "out", (2, 16, 64), 64, 2, 1, ("t2",)),
    Route("t2-k3", "function", "out", (2, 16, 64), 64, 2, 3, ("t2",)),
    Route("wide256-out", "function", "out", (2, 16, 64), 256, 3, 3, ("wide-max",)),
    Route("wide256-out-k1", "function", "out", (2, 16, 64), 256, 4, 1, ("wide-max",)),
    Route("wide256-in", "function", "in", (2, 16, 64), 256, 4, 3, ("wide-max",)),
    Route("wide256-in-k1", "function", "in", (2, 16, 64), 256, 4, 1, ("wide-max",)),
    Route("wide160-out", "function", "out", (2, 16, 64), 160, 3, 3, ("wide-odd",)),                   # (takes_out refuses k = 1 at 160 and 96)
    Route("wide96-in", "function", "in", (2, 16, 64), 96, 4, 3, ("wide-odd",)),                       # (takes_in refuses k = 1 at 96)
] + _abi("grad_weight", [(3, 5, 12), (5, 3, 20), (4, 3, 4), (2, 3, 4), (1, 1, 4), (1, 7, 33), (1, 4, 1), (1, 2, 2)], {
    (3, 5, 12): ("ystep", "carry-period", "t2"),                                                       # the walk (8, 2)
    (5, 3, 20): ("ystep", "carry-period", "t2"),                                                       # (12, 1)
    (4, 3, 4): ("ystep", "double-wrap", "t2"),                                                         # (0, 8): y passes 2 H on every second pixel
    (2, 3, 4): ("empty-groups", "t2"),                                                                 # 24 pixels: no thread takes a second one
    (1, 1, 4): ("empty-groups", "all-border", "t2"),
    (1, 7, 33): ("carry-period", "t2"),                                                                # (32, 0): a carry on all steps but one in 33
    (1, 4, 1): ("empty-groups", "all-border", "t2"),                                                   # H = 4 rows of one pixel
    (1, 2, 2): ("empty-groups", "all-border", "t2"),
}) + [Route("grad_weight-96", "grad_weight", "both", (3, 5, 12), 96, 3, 3, ("ystep", "carry-period", "wide-odd"))] + _abi(
    "expand", [(3, 5, 12), (1, 1, 4), (2, 3, 4), (5, 3, 20)], {
        (3, 5, 12): ("straddle", "short-tail", "row-mod", "t2"),
        (1, 1, 4): ("short-tail", "one-window", "t2"),
        (2, 3, 4): ("straddle", "short-tail", "row-mod", "one-window", "t2"),
        (5, 3, 20): ("straddle", "short-tail", "row-mod", "t2"),
    }) + [Route("expand-160", "expand", "out", (3, 5, 12), 160, 3, 3, ("straddle", "short-tail", "row-mod", "wide-odd"))]
ABI_T, ABI_K = (1, 2, 3, 4), (1, 3)      # what an entry-point case is run at, besides its own (T, k)

# ps_thin_add_bias_f32 on flat buffers: (npix, C, y aligned to 16 bytes) -> the branches of BIAS_BRANCHES it reaches
BIAS_BRANCHES = {"loops": bias_loops, "stride-turns": bias_stride_turns, "scalar-c4": bias_scalar_c4, "partial-block": bias_partial_block,
                 "other-c": lambda npix, C, aligned: C % 4 != 0 and C not in (1, 3)}
BIAS_ROUTES = [
    ((65600, 128, True), ("loops",)),                          # the float4 loop's second pass
    ((87400, 96, True), ("loops", "stride-turns")),            # ... with a stride of 2^21 float4s on pixels of 24
    ((699100, 3, True), ("loops", "stride-turns", "partial-block")),      # the scalar loop's second pass
    ((1000, 8, False), ("scalar-c4", "partial-block")),        # y four bytes off: the scalar kernel at a C that is a multiple of 4
    ((1000, 5, True), ("other-c", "partial-block")),
    ((1, 1, True), ("partial-block",)),                        # one thread (C = 1 itself is run by THIN_OUT's 1 at k = 3)
]


def old_cases():
    """Every (kind, frame, wide, T, k) the operator, block and decoder tests of tests/test_thin_train_gpu.py run the kernels at"""
    out = [("out", f, w, T, k) for f in FRAMES for w in WIDE for T in THIN_OUT for k in KS] + [("out", RAGGED, 32, 3, 3), ("out", RAGGED, 128, 4, 1)]
    out += [("in", f, w, 4, k) for f in FRAMES for w in WIDE for k in KS] + [("in", RAGGED, 32, 4, 3), ("in", RAGGED, 64, 4, 1)]
    out += [("out", (10, 8, 64), 32, T, k) for T, k in ((1, 3), (3, 3), (4, 3), (3, 1))]              # the one-hot gradient, a spot per frame
    out += [("in", (2, 8, 64), 64, 4, 3), ("out", (2, 8, 64), 64, 3, 3)]                              # the one-hot pairs
    out += [(kind, (2, 8, 64), w, T, k) for kind, w, T in (("in", 64, 4), ("out", 128, 3)) for k in KS]      # the two thin blocks
    out += [("out", (1, 64, 64), 128, 3, k) for k in KS]                                              # the decoder
    return out + [(kind, (1,) + f[1:], w, T, k) for kind, f, w, T, k in out if kind == "out" and f[0] > 1]      # the last frame alone


def old_bias_calls():
    """(npix, C, aligned) of every ps_thin_add_bias_f32 call those tests make: the 3 x 3 layers' outputs, torch's allocations (aligned)"""
    return sorted({(f[0] * f[1] * f[2], w if kind == "in" else T, True) for kind, f, w, T, k in old_cases() if k == 3})


def inputs(kind, frame, wide, T, k, seed=0):
    """x (B, Ci, H, W), w (Co, Ci, k, k), b (Co), g (B, Co, H, W) of a thin-in (4 -> wide) or thin-out (wide -> T) layer"""
    B, H, W = frame
    Ci, Co = (4, wide) if kind == "in" else (wide, T)
    gen = torch.Generator().manual_seed(seed + 7 * B + H + W + wide + 13 * T + k)
    return (torch.randn(B, Ci, H, W, generator=gen), torch.randn(Co, Ci, k, k, generator=gen) * (Ci * k * k) ** -0.5,
            torch.randn(Co, generator=gen), torch.randn(B, Co, H, W, generator=gen))
