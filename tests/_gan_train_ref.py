"""What the tests of the discriminator's training kernels (csrc/gan_train.hip, networks/gan_train.py) compare against: the fp64 formulas
of include/pixelsynth_gan_train.h, its constants, and the bounds.

Bounds.  u = 2^-24 bounds the relative error of one fp32 rounding; n = HW values per plane; m2 = S2 / n.

  mean     the fp64 sum is rounded once:                                    |mean - mean64| <= u |mean64|
  var      rounded once; in front of it the fp64 difference m2 - mean^2 of two numbers of size m2, each known to a few n 2^-53 of its
           size.  The issue sets 2^-40 m2 for that term at every size tested here (n <= 8281: the worst case of any order of summation
           would be 2 n 2^-53 = 2^-39, a sum that errs with one sign at every step; the term is kept as set):
                                                                            |var - var64| <= u var64 + 2^-40 m2
  rstd     (the kernel's var is not an output: it shows in rstd) = (var + eps)^-1/2, so a relative error e of var + eps is e / 2 of
           rstd: the var bound above, the rounding of the fp32 sum var + eps (u), both halved, and rstd's own rounding (u):
                                                     |rstd - rstd64| <= rstd64 (var_bound / (2 (var64 + eps)) + 1.5 u) (1 + 2^-10)
           (the last factor: the second-order terms).  The fp32 m2 - mean^2 misses this on a plane of 100 + 0.01 randn by orders.
  y        the five rounded operations on the way from the fp64 statistics to y, r = rstd64, c = x - mean64, v = c r:
             mean          1 rounding                                       u |mean| r
             x - mean      its rounding                                     u |c| r
             rstd          1.5 u + the fp64 term t = 2^-40 m2 / (2 (var64 + eps)) as above, rounded up:   (2 u + t) |v|
             c * rstd      its rounding                                     u |v|
             v * slope     its rounding (slope < 1, or nothing on the other branch)                       u |v|
           |c| <= |x| + |mean| and |v| <= (|x| + |mean|) r, so together 6 u (|x| + |mean|) r + t |v|:  C_Y = 6.  Both branches of the
           LeakyReLU have slope <= 1, so an element whose v changes sign between the kernel and fp64 is within the same bound.
  feat     d = f - r in fp32 in the reference too (the kernel's own first step, exact as a definition); the fp64 sum of n terms is off
           by at most n 2^-53 of it in any order, the kernel's and the reference's: n 2^-52 between them; one rounding to fp32:
                                                                            |per_map - S64 / n| <= (u + n 2^-52) S64 / n
           and the same for the total, with sum_k |w_k| S_k / n_k in place of S64 / n.
  g        the project's rule for gradients: |g - g64| <= 4 max(E32, 1e-6 max |g64|), E32 the largest error of torch's fp32 evaluation
           of the same formula on the host (grad_bound).  For dx the fp64 reference takes the LeakyReLU's branch from the sign of the
           kernel's own y (which the y bound holds to the fp64 value's sign wherever it matters), so no element is left out.
"""
import numpy as np
import torch
import torch.nn.functional as F

WAVE_HW, RESIDENT_HW, MAX_MAPS, TILE = 2048, 8192, 16, 16384      # PS_GAN_TRAIN_* of the header (tests/test_gan_train_cpu.py holds them to it)
U = 2.0 ** -24
C_Y = 6


def form(hw):
    """Which kernel takes a plane of hw values, and the values a thread holds (the header's table)"""
    if hw <= WAVE_HW:
        return "wave", 4 * -(-(-(-hw // 64)) // 4)
    if hw <= RESIDENT_HW:
        return "workgroup", 4 * -(-(-(-hw // 256)) // 4)
    return "stream", 0


# The boundaries of values_per_thread that the operator cases of tests/test_gan_train_gpu.py leave on both sides: hw | hw + 1 are two
# forms.  Both sides of each are a route case (test_disc_routes_cpu.py, test_disc_routes_gpu.py): five planes up to 1793 values, so that
# the wave form's last workgroup has one wavefront at work, two planes above.  They reach k_norm_fwd / k_norm_bwd <64, NV> at
# NV = 12, 16, 24, 28 and <256, NV> at NV = 24, 28, the six instantiations no other test launches, twice each.
NORM_ROUTE_BOUNDARIES = [512, 768, 1024, 1280, 1536, 1792, 4096, 5120, 6144, 7168]
NORM_ROUTE_CASES = [(1, 5 if hw <= 1793 else 2, 1, hw) for b in NORM_ROUTE_BOUNDARIES for hw in (b, b + 1)]
NORM_ROUTE_FORMS = [("wave", 12), ("wave", 16), ("wave", 24), ("wave", 28), ("workgroup", 24), ("workgroup", 28)]
# k_feat_finish stages the tiles of a map 256 at a time: a map of more than 256 tiles takes a second trip round the reused `stage`.
# "staged": 258 tiles (a full trip, a trip of 2, a ragged last tile), then maps whose first tiles are at no multiple of 256;
# "staged-exact": two full trips
FEAT_STAGE = 256
FEAT_ROUTE_LISTS = {"staged": [(2, 257 * TILE + 3), (2, 5), (2, TILE)], "staged-exact": [(2, 512 * TILE)]}


def feat_tiles(shapes):
    """Tiles per map of a list of map shapes (2P, ...): ceil(values per half / TILE)"""
    out = []
    for s in shapes:
        n = 1
        for v in s:
            n *= v
        out.append(-(-(n // 2) // TILE))
    return out


def norm_inputs(shape, seed=0):
    """x = 0.3 + 1.5 randn and dy = randn, as the tests draw them"""
    gen = torch.Generator().manual_seed(seed)
    return 0.3 + 1.5 * torch.randn(*shape, generator=gen), torch.randn(*shape, generator=gen)


def norm_forward64(x, eps, slope):
    """The header's forward in fp64 on the fp32 input -> dict(mean, var, m2, rstd (B, C), v, y (B, C, H, W))"""
    x = x.double()
    mean, m2 = x.mean((2, 3)), (x * x).mean((2, 3))
    var = (m2 - mean * mean).clamp_min(0)
    rstd = (var + eps).rsqrt()
    v = (x - mean[:, :, None, None]) * rstd[:, :, None, None]
    return dict(mean=mean, var=var, m2=m2, rstd=rstd, v=v, y=torch.where(v > 0, v, v * slope))


def norm_backward64(x, dy, eps, slope, y=None):
    """The header's backward in fp64; the LeakyReLU's branch from the sign of `y` (the kernel's own output) where given"""
    f = norm_forward64(x, eps, slope)
    v, dy = f["v"], dy.double()
    pos = (v if y is None else y.double().cpu()) > 0
    g = torch.where(pos, dy, dy * slope)
    m1, m2 = g.mean((2, 3), keepdim=True), (g * v).mean((2, 3), keepdim=True)
    return f["rstd"][:, :, None, None] * (g - m1 - v * m2)


def norm_autograd(x, dy, eps, slope, dtype):
    """dx of sum(LeakyReLU(InstanceNorm(x)) * dy) by torch autograd in `dtype` on the host; the normalisation written out (the biased
    variance about the mean): F.instance_norm refuses a plane of one value"""
    x = x.detach().cpu().to(dtype).clone().requires_grad_()
    c = x - x.mean((2, 3), keepdim=True)
    v = c * (c * c).mean((2, 3), keepdim=True).add(eps).rsqrt()
    (F.leaky_relu(v, slope) * dy.cpu().to(dtype)).sum().backward()
    return x.grad


def stat_bounds(f, eps):
    """-> the bounds of mean and rstd (B, C), and the fp64 term t of the docstring"""
    var_bound = U * f["var"] + 2.0 ** -40 * f["m2"]
    rel = var_bound / (2 * (f["var"] + eps))
    return U * f["mean"].abs(), f["rstd"] * (rel + 1.5 * U) * (1 + 2.0 ** -10), 2.0 ** -40 * f["m2"] / (2 * (f["var"] + eps))


def y_bound(x, f, eps):
    t = stat_bounds(f, eps)[2][:, :, None, None]
    return C_Y * U * (x.double().abs() + f["mean"].abs()[:, :, None, None]) * f["rstd"][:, :, None, None] + t * f["v"].abs()


def feat_maps(shapes, seed=0, ties=True):
    """Maps (2P, ...) of randn, as the tests draw them; with `ties`, every 7th value of the fake half equals its real partner"""
    gen = torch.Generator().manual_seed(seed)
    maps = [torch.randn(*s, generator=gen) for s in shapes]
    if ties:
        for m in maps:
            half = m.size(0) // 2
            m[:half].reshape(-1)[::7] = m[half:].reshape(-1)[::7]
    return maps


def feat_forward64(maps, weights):
    """-> per_map (fp64 means of |f - r|, the difference in fp32), total, and the total of the magnitudes (for its bound)"""
    per = []
    for m in maps:
        m = m.detach().cpu()
        half = m.size(0) // 2
        per.append((m[:half] - m[half:]).abs().double().sum().item() / (m.numel() // 2))
    return per, sum(w * p for w, p in zip(weights, per)), sum(abs(w) * p for w, p in zip(weights, per))


def feat_value_bound(n, magnitude):
    return (U + n * 2.0 ** -52) * magnitude


def feat_backward32(maps, weights, grad_total):
    """The header's backward as it rounds: s_k = fp32(double(grad_total) w_k / n_k), s_k sgn(d) into the fake half, +0 into the real"""
    out = []
    for m, w in zip(maps, weights):
        m = m.detach().cpu()
        half, n = m.size(0) // 2, m.numel() // 2
        s = np.float32(np.float64(np.float32(grad_total)) * np.float64(w) / np.float64(n))
        g = torch.zeros_like(m)
        g[:half] = torch.sign(m[:half] - m[half:]) * torch.tensor(s)
        out.append(g)
    return out


def grad_bound(g32, g64):
    """-> (bound, E32)"""
    E32 = (g32.double() - g64).abs().max().item()
    return 4 * max(E32, 1e-6 * g64.abs().max().item()), E32


def check(name, got, want, bound):
    """max |got - want| / bound, printed; bound a number or a tensor of want's shape"""
    got = got.detach()
    err = (got.double().cpu() - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    assert got.shape == want.shape and torch.isfinite(got).all(), name
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: max |err| {err.max().item():.3e}, error / bound {ratio:.3f}")
    return ratio
