"""What the tests of the training-mode batch norm (csrc/norm_train.hip, networks/norm_train.py) compare against: the fp64 formulas of
include/pixelsynth_norm_train.h, the mirror of its split into parts, and the bounds.

Bounds.  u = 2^-24 bounds the relative error of one fp32 rounding.

  mean     the fp64 sum is rounded once:                                   |mean - mean64| <= u |mean64|
  var      rounded once; in front of it the fp64 difference m2 - mean^2 of two numbers of size m2, each known to a few N 2^-53 of its
           size (N <= 2^12 rows here gives 2^-41; 2^-40 holds it):         |var - var64|  <= u var64 + 2^-40 m2_64
           For N rows beyond 2^12 (the route cases below; stat_bounds(x, rows=N)): a sum of N terms in fp64 is off by at most N 2^-53 of
           the sum of their magnitudes in ANY order, so the kernel's m2 and mean^2 carry N 2^-53 m2 each at the most, and so do the
           reference's (torch's own order): 2 N 2^-53 m2 between them, and the term is  max(2^-40, N 2^-52) m2_64.
  y        the path from the fp64 statistics to y, written s = scale64, m = mean64:
             mean         1 rounding                                        u
             rstd         var's rounding and that of var + eps are halved by the root (u together), its own rounding: 2 u
             scale        rstd * gain, one more:                            3 u
             x * scale    one more:                                         4 u |x s|
             mean * scale u + 3 u + its own:                                5 u |m s|
             shift        the difference's rounding:                        u |shift|
             y            the last difference's rounding, u |y| <= u (|x s| + |shift|)
           together 5 u |x s| + 5 u |m s| + 2 u |shift| <= 5 u (|x s| + |shift| + |m s|); with the second-order terms C_FWD = 6 -- the
           six roundings on the longest path: the fp32 mean, rstd, two products, two differences.
  g        the project's rule for gradients: |g - g64| <= 4 max(E32, 1e-6 max |g64|), E32 the largest error of torch's fp32 autograd of
           the same formula on the host (grad_bound).
"""
from collections import namedtuple

import torch

MAX_PARTS, PART_ROWS, MAX_C = 512, 512, 65536       # PS_NORM_TRAIN_* of the header (tests/test_norm_train_cpu.py holds them to it)
U = 2.0 ** -24
C_FWD = 6
assert C_FWD <= 8


def sizes_ok(B, HW, C):
    return B >= 1 and HW >= 1 and C >= 1 and C % 4 == 0 and C <= MAX_C and HW * C < 2 ** 31 and B * HW < 2 ** 31


def part_rows(B, HW):
    per_frame = max(1, MAX_PARTS // B)
    return PART_ROWS * -(-(-(-HW // PART_ROWS)) // per_frame)


def part_ranges(B, HW):
    """[(frame, first row, end row)] of the parts in their order: consecutive rows of one frame each"""
    rows = part_rows(B, HW)
    return [(b, r, min(r + rows, HW)) for b in range(B) for r in range(0, HW, rows)]


# ---- the rest of the plan (csrc/norm_train.hip: make_plan, lane_of, walk, sum_parts; the header states the formulas) ----------------------
THREADS, MAX_CW, DEPTH = 256, 64, 4                 # threads of a workgroup; float4s of channels it takes at most; rows a thread has in flight
FIN_CH, FIN_PARTS = 32, 64                          # channels of a finishing workgroup; parts sum_parts stages at a time

Plan = namedtuple("Plan", "C4 cw rl idle chunks last_cw part_rows ppf parts fin_wgs last_fin")


def plan(B, HW, C):
    """cw channel quads times rl row lanes per workgroup (idle: the threads left over), `chunks` workgroups across the channels, the last
    with last_cw quads; ppf parts per frame; fin_wgs finishing workgroups of 32 channels, the last with last_fin"""
    C4 = C // 4
    cw = min(C4, MAX_CW)
    rl, chunks = THREADS // cw, -(-C4 // cw)
    rows = part_rows(B, HW)
    ppf = -(-HW // rows)
    fin = -(-C // FIN_CH)
    return Plan(C4, cw, rl, THREADS - cw * rl, chunks, C4 - (chunks - 1) * cw, rows, ppf, B * ppf, fin, C - (fin - 1) * FIN_CH)


def batches(p0, p1):
    """[(first part, parts)] of the batches sum_parts stages for the parts p0 .. p1 - 1: FIN_PARTS at a time from p0"""
    return [(b, min(FIN_PARTS, p1 - b)) for b in range(p0, p1, FIN_PARTS)]


def walk(r0, r1, rl):
    """walk() restated for a lane whose rows are r0, r0 + rl, ... < r1 -> (exit, steps, tail, loads, uses): which register set the
    double-buffered loop used last ("none": it never ran, "set0", "set1"), how many blocks of DEPTH rows it used, how many rows the
    one-at-a-time loop took after it; the rows loaded and the rows used, in order"""
    step, last = DEPTH * rl, (DEPTH - 1) * rl
    r, exit_, steps, loads, uses = r0, "none", 0, [], []
    rows = lambda a: [a + d * rl for d in range(DEPTH)]
    if r + last < r1:
        loads += rows(r)
        while True:
            more = r + step + last < r1
            if more:
                loads += rows(r + step)
            uses += rows(r)
            steps, r = steps + 1, r + step
            if not more:
                exit_ = "set0"
                break
            more = r + step + last < r1
            if more:
                loads += rows(r + step)
            uses += rows(r)
            steps, r = steps + 1, r + step
            if not more:
                exit_ = "set1"
                break
    tail = list(range(r, r1, rl))
    return exit_, steps, len(tail), loads + tail, uses + tail


def walk_kinds(B, HW, C):
    """{(exit, min(steps, 3), tail)} over every lane of every part of a frame (the frames are alike); asserts on the way that each lane
    loads and uses exactly its rows, each once, in ascending order -- no prefetch past the part"""
    p, kinds = plan(B, HW, C), set()
    for _, r0, r1 in (q for q in part_ranges(B, HW) if q[0] == 0):
        for lane in range(p.rl):
            e, steps, tail, loads, uses = walk(r0 + lane, r1, p.rl)
            assert loads == uses == list(range(r0 + lane, r1, p.rl)), (B, HW, C, r0, lane)
            kinds.add((e, min(steps, 3), tail))
    return kinds


RouteCase = namedtuple("RouteCase", "id shape why")          # shape (B, C, H, W)
ROUTE_CASES = [
    RouteCase("chunk_tail", (1, 260, 6, 8), "chunks = 2, the last chunk one quad; 9 finishing workgroups, the last with 4 channels"),
    RouteCase("chunks_full", (2, 512, 8, 8), "the decoder's widest norm: two full chunks"),
    RouteCase("many_frames", (130, 8, 1, 3), "parts = 130: three batches (64, 64, 2) in k_stats_finish; lanes with no row"),
    RouteCase("many_parts_per_frame", (2, 4, 130, 256), "ppf = 65: two batches in k_bwd_frames, frame 1 starts at part 65"),
    RouteCase("long_parts", (256, 4, 25, 41), "part_rows = 1024, parts = 512 = the maximum, eight full batches; a last part of one row"),
    RouteCase("idle_lane_tails", (2, 12, 25, 28), "cw = 3, rl = 85, one idle thread; tails 2 and 3 with and without a pipelined block"),
    RouteCase("two_step_tails", (1, 20, 26, 50), "cw = 5, rl = 51, ppf = 3; the loop left after set 1 with exactly 2 steps, tails 2 and 3"),
    RouteCase("deep_tails", (1, 36, 24, 38), "cw = 9, rl = 28, four idle threads; tails 2 and 3 after >= 3 steps from either set"),
    RouteCase("single_value", (1, 4, 1, 1), "n = 1: var = 0, two equal terms cancel in dx"),
]
# (B, C, H, W) of the operator tests of tests/test_norm_train_gpu.py: its CASES, the ill-conditioned / NaN shape, and the norms of its
# unresampled blocks
OPERATOR_SHAPES = [(3, 4, 20, 12), (2, 64, 32, 32), (1, 192, 16, 16), (2, 128, 48, 80), (2, 8, 16, 16), (2, 128, 32, 32), (2, 16, 16, 16)]


def inputs(B, C, H, W, seed=0, shared=False):
    """x, gain, bias, dy as the tests draw them: x = 0.3 + 1.5 randn, gain = 1 + 0.3 randn, bias = 0.3 randn ((1, C) when shared)"""
    gen = torch.Generator().manual_seed(seed)
    x = 0.3 + 1.5 * torch.randn(B, C, H, W, generator=gen)
    rows = 1 if shared else B
    gain = 1 + 0.3 * torch.randn(rows, C, generator=gen)
    bias = 0.3 * torch.randn(rows, C, generator=gen)
    dy = torch.randn(B, C, H, W, generator=gen)
    return x, gain, bias, dy


def _bc(t):
    return t.reshape(t.size(0), -1, 1, 1)


def stats64(x):
    """mean, var (biased, clamped at 0) and the mean of squares per channel, fp64"""
    x = x.double()
    m, m2 = x.mean((0, 2, 3)), (x * x).mean((0, 2, 3))
    return m, (m2 - m * m).clamp_min(0), m2


def forward64(x, gain, bias, eps, relu):
    """The header's forward formulas in fp64 on the fp32 inputs -> dict(mean, var, m2, scale, shift, v, y)"""
    m, var, m2 = stats64(x)
    scale = torch.rsqrt(var + eps).view(1, -1, 1, 1) * _bc(gain.double())
    shift = m.view(1, -1, 1, 1) * scale - _bc(bias.double())
    v = x.double() * scale - shift
    return dict(mean=m, var=var, m2=m2, scale=scale, shift=shift, v=v, y=v.clamp_min(0) if relu else v)


def backward64(x, dy, gain, bias, eps, relu):
    """The header's backward formulas in fp64 -> dx (B, C, H, W), dgain, dbias (B, C): per-frame sums, two per-channel means, one pass"""
    f = forward64(x, gain, bias, eps, relu)
    x, dy, gain = x.double(), dy.double(), _bc(gain.double())
    g = torch.where(f["v"] > 0, dy, torch.zeros_like(dy)) if relu else dy
    rstd = torch.rsqrt(f["var"] + eps).view(1, -1, 1, 1)
    xhat = (x - f["mean"].view(1, -1, 1, 1)) * rstd
    dbias, dgain = g.sum((2, 3)), (g * xhat).sum((2, 3))
    n = x.size(0) * x.size(2) * x.size(3)
    k1 = (gain * _bc(dbias)).sum(0, keepdim=True) / n
    k2 = (gain * _bc(dgain)).sum(0, keepdim=True) / n
    return rstd * (gain * g - k1 - xhat * k2), dgain, dbias


def composition(x, gain, bias, eps, relu):
    """The reference's composition for autograd, in x's precision: the m2 - m^2 statistics, x * scale - shift"""
    m = x.mean((0, 2, 3), keepdim=True)
    var = (x * x).mean((0, 2, 3), keepdim=True) - m * m
    scale = torch.rsqrt(var + eps) * _bc(gain)
    y = x * scale - (m * scale - _bc(bias))
    return torch.relu(y) if relu else y


def autograd(x, gain, bias, dy, eps, relu, dtype):
    """(dx, dgain, dbias) of sum(composition * dy) by torch autograd in `dtype` on the host; gain / bias keep their (B or 1, C) shape"""
    x, gain, bias = (t.detach().to(dtype).clone().requires_grad_() for t in (x, gain, bias))
    (composition(x, gain, bias, eps, relu) * dy.to(dtype)).sum().backward()
    return x.grad, gain.grad, bias.grad


def stat_bounds(x, rows=None):
    """-> (mean's bound, var's); rows = N = B HW for cases past 2^12 rows: the m2 term grows to max(2^-40, N 2^-52) (the docstring)"""
    m, var, m2 = stats64(x)
    return U * m.abs(), U * var + (2.0 ** -40 if rows is None else max(2.0 ** -40, rows * 2.0 ** -52)) * m2


def forward_bound(x, f):
    return C_FWD * U * ((x.double() * f["scale"]).abs() + f["shift"].abs() + (f["mean"].view(1, -1, 1, 1) * f["scale"]).abs())


def grad_bound(g32, g64):
    """-> (bound, E32)"""
    E32 = (g32.double() - g64).abs().max().item()
    return 4 * max(E32, 1e-6 * g64.abs().max().item()), E32


def check(name, got, want, bound):
    """max |got - want| / bound, printed; bound a number or a tensor of want's shape"""
    err = (got.double().cpu() - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    assert got.shape == want.shape and torch.isfinite(got).all(), name
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: max |err| {err.max().item():.3e}, error / bound {ratio:.3f}")
    return ratio
