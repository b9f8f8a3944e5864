"""What the tests of the batched spectral normalisation (csrc/spectral_train.hip, networks/spectral_train.py) compare against: the fp64
mirror of include/pixelsynth_spectral_train.h on the fp32 inputs, torch's own fp32 arithmetic of the legacy hook on the host, the
header's constants and plan, and the bounds.

Bounds.  U = 2^-24 bounds the relative error of one fp32 rounding.  The kernels take every sum over a row or a column in fp64 and keep
what is not stored (t, |t|, s, |s|) in fp64; a STORED value (v, u, sigma, W_sn, dW) is one rounding of its fp64 expression.  A fp64 sum
of n products errs by at most n 2^-53 of the sum of their magnitudes in any order, and 2^-52 n is taken (the reference's own sum is one
such order).  |A| is the matrix of magnitudes.  Every bound is per element:

  t = W^T u     fp64:                                             e_t = R 2^-52 |W|^T |u|
  n = |t|       fp64; the norm moves by at most the norm of the error of its argument:
                                                                  e_n = |e_t|_2 + C 2^-52 n
  v = t / n     stored, one rounding:                             e_v = e_t / n + |v| (e_n / n + U)
  s = W v       fp64; the stored v, not the reference's, goes in: e_s = |W| e_v + C 2^-52 |W| |v|
  m = |s|       fp64:                                             e_m = |e_s|_2 + R 2^-52 m
  u = s / m     stored, one rounding:                             e_u = e_s / m + |u| (e_m / m + U)
  sigma = u . s                                                   e_sigma = e_u . |s| + |u| . e_s + U |sigma| + R 2^-52 |u| . |s|
  W_sn = W / sigma                                                e_w = |W_sn| (e_sigma / |sigma| + U)
  (a layer that does not iterate: e_v = e_u = 0, they are the inputs)
  d = sum G W_sn                                                  e_d = |G| . e_w + U |d| + R C 2^-52 |G| . |W_sn|
  p = (d u_r) v_c   two roundings:                                e_p = e_d |u| |v| + |d| (e_u |v| + |u| e_v) + 2 U |d u v|
  dW = (G - p) / sigma   the difference's and the quotient's rounding:
                                                                  e_dW = (e_p + U |G - p|) / |sigma| + |dW| (e_sigma / |sigma| + U)
each times (1 + 2^-10) for the terms of second order.  Above these stands the project's ceiling, which no bound may exceed:
4 max(E32, 1e-6 max |y64|), E32 the largest error of torch's own fp32 arithmetic of the hook on the host (hook32, autograd32); the bound
of a value is the smaller of the two, element by element (bounded()).
"""
import torch
import torch.nn.functional as F

MAX_LAYERS, PART_ROWS, TILE, FORWARD_LAUNCHES, BACKWARD_LAUNCHES = 64, 16, 4096, 5, 2     # PS_SPECTRAL_* of the header
U = 2.0 ** -24
SECOND = 1 + 2.0 ** -10
EPS = 1e-12

# (R, C) of the issue, and the pairs on both sides of the plan's boundaries: a part of 16 rows (16 | 17), a group of four rows (4 | 5), a
# tile of 4096 values (64 x 64 | 64 x 65), the 1024 columns a workgroup of k_sn_wtu covers per round and the 256 a wavefront of k_sn_wv
# does (1024 | 1028 | 1025: the last with a scalar tail), the 256 entries a workgroup's threads cover per round (256 | 257 rows)
SHAPES = [(3, 27), (64, 20), (1, 576), (16, 64), (5, 7), (130, 300), (2, 4608), (512, 64)]
BOUNDARY_SHAPES = [(17, 64), (4, 9), (64, 65), (3, 1024), (3, 1028), (3, 1025), (256, 8), (257, 8)]


def plan(R, C):
    """(parts of W^T u, groups of four rows, tiles) of a layer: the header's plan"""
    return -(-R // PART_ROWS), -(-R // 4), -(-(R * C) // TILE)


def workspace_bytes(shapes):
    """The header's workspace: the parts of W^T u and a double per tile, then the rows of s as doubles, each region a multiple of 256"""
    up = lambda n: -(-n // 256) * 256
    return (up(8 * sum(plan(R, C)[0] * C for R, C in shapes)) + up(8 * sum(plan(R, C)[2] for R, C in shapes))
            + up(8 * sum(R for R, _ in shapes)))


def layer_inputs(R, C, seed=0, scale=0.05):
    """W = scale randn (R, C), u and v unit vectors, as the tests draw them (fp32)"""
    gen = torch.Generator().manual_seed(seed * 7919 + R * 131 + C)
    W = scale * torch.randn(R, C, generator=gen)
    return W, F.normalize(torch.randn(R, generator=gen), dim=0), F.normalize(torch.randn(C, generator=gen), dim=0)


def forward64(W, u, v, iterate, eps=EPS):
    """The header's forward in fp64 on the given (fp32) inputs -> dict(v, u, s, sigma, w) in fp64"""
    W, u, v = W.detach().cpu().double().reshape(W.size(0), -1), u.detach().cpu().double(), v.detach().cpu().double()
    if iterate:
        t = W.t() @ u
        v = t / t.norm().clamp_min(eps)
        s = W @ v
        u = s / s.norm().clamp_min(eps)
    else:
        s = W @ v
    sigma = u @ s
    return dict(v=v, u=u, s=s, sigma=sigma, w=W / sigma)


def backward64(f, G):
    """The header's backward in fp64 from forward64's dict: dW = (G - d u v^T) / sigma, d = sum G W_sn"""
    G = G.detach().cpu().double().reshape(f["w"].shape)
    d = (G * f["w"]).sum()
    return (G - d * torch.outer(f["u"], f["v"])) / f["sigma"]


def hook(W, u, v, iterate, eps=EPS):
    """torch's arithmetic of the legacy hook (SpectralNorm.compute_weight, n_power_iterations = 1, dim = 0) in the dtype of W, u and v
    updated IN PLACE where it iterates; -> (W_sn, sigma) in the graph of W"""
    Wm = W.reshape(W.size(0), -1)
    if iterate:
        with torch.no_grad():
            v.copy_(F.normalize(torch.mv(Wm.t(), u), dim=0, eps=eps))
            u.copy_(F.normalize(torch.mv(Wm, v), dim=0, eps=eps))
        u, v = u.clone(), v.clone()
    sigma = torch.dot(u, torch.mv(Wm, v))
    return W / sigma, sigma


def hook32(W, u, v, iterate, eps=EPS):
    """hook() in fp32 on the host on copies -> dict(v, u, sigma, w)"""
    W, u, v = (t.detach().cpu().float().clone() for t in (W, u, v))
    w, sigma = hook(W.reshape(W.size(0), -1), u, v, iterate, eps)
    return dict(v=v, u=u, sigma=sigma, w=w)


def autograd(W, u, v, iterate, G, dtype, eps=EPS):
    """dW of sum(hook's W_sn * G) by torch autograd in `dtype` on the host"""
    W = W.detach().cpu().to(dtype).reshape(W.size(0), -1).clone().requires_grad_()
    w, _ = hook(W, u.detach().cpu().to(dtype).clone(), v.detach().cpu().to(dtype).clone(), iterate, eps)
    (w * G.detach().cpu().to(dtype).reshape(w.shape)).sum().backward()
    return W.grad


def forward_errors(W, u, v, iterate, f):
    """The derived bounds of the docstring for forward64's dict f -> dict(v, u, s, sigma, w)"""
    A = W.detach().cpu().double().reshape(W.size(0), -1).abs()
    R, C = A.shape
    if iterate:
        u_in = u.detach().cpu().double()
        t = W.detach().cpu().double().reshape(R, C).t() @ u_in
        n = t.norm()
        e_t = R * 2.0 ** -52 * (A.t() @ u_in.abs())
        e_n = e_t.norm() + C * 2.0 ** -52 * n
        e_v = e_t / n + f["v"].abs() * (e_n / n + U)
    else:
        e_v = torch.zeros(C, dtype=torch.float64)
    e_s = A @ e_v + C * 2.0 ** -52 * (A @ f["v"].abs())
    if iterate:
        m = f["s"].norm()
        e_m = e_s.norm() + R * 2.0 ** -52 * m
        e_u = e_s / m + f["u"].abs() * (e_m / m + U)
    else:
        e_u = torch.zeros(R, dtype=torch.float64)
    sigma = f["sigma"].abs()
    e_sigma = e_u @ f["s"].abs() + f["u"].abs() @ e_s + U * sigma + R * 2.0 ** -52 * (f["u"].abs() @ f["s"].abs())
    e_w = f["w"].abs() * (e_sigma / sigma + U)
    return {k: e * SECOND for k, e in dict(v=e_v, u=e_u, s=e_s, sigma=e_sigma, w=e_w).items()}


def backward_error(f, e, G, dW):
    """The derived bound of dW (backward64's) from forward64's f and forward_errors' e"""
    G = G.detach().cpu().double().reshape(f["w"].shape)
    R, C = G.shape
    d = (G * f["w"]).sum().abs()
    e_d = (G.abs() * e["w"]).sum() + U * d + R * C * 2.0 ** -52 * (G.abs() * f["w"].abs()).sum()
    au, av = f["u"].abs(), f["v"].abs()
    uv = torch.outer(au, av)
    e_p = e_d * uv + d * (torch.outer(e["u"], av) + torch.outer(au, e["v"])) + 2 * U * d * uv
    sigma = f["sigma"].abs()
    p = (G * f["w"]).sum() * torch.outer(f["u"], f["v"])
    return ((e_p + U * (G - p).abs()) / sigma + dW.abs() * (e["sigma"] / sigma + U)) * SECOND


def ceiling(y32, y64):
    """The project's rule: 4 max(E32, 1e-6 max |y64|) -> (ceiling, E32)"""
    y64 = torch.as_tensor(y64, dtype=torch.float64)
    E32 = (torch.as_tensor(y32).double().reshape(y64.shape) - y64).abs().max().item()
    return 4 * max(E32, 1e-6 * y64.abs().max().item()), E32


def bounded(derived, y32, y64):
    """The bound of a value: the derived one, element by element, and never more than the ceiling"""
    return torch.as_tensor(derived, dtype=torch.float64).clamp_max(ceiling(y32, y64)[0])


def check(name, got, want, bound):
    """max |got - want| / bound, printed; bound a number or a tensor of want's shape.  Every element counts"""
    got, want = torch.as_tensor(got).detach().double().cpu(), torch.as_tensor(want, dtype=torch.float64)
    got = got.reshape(want.shape)
    assert torch.isfinite(got).all(), name
    err = (got - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: max |err| {err.max().item():.3e}, error / bound {ratio:.3f}")
    return ratio


def simulate(W, u, v, iterate, eps=EPS):
    """The kernels' arithmetic on the host, but for the order of the fp64 sums: t, |t|, s, |s| in fp64, every stored value an fp64
    expression rounded once to fp32 -> dict(v, u, sigma, w) in fp32.  What the CPU tests hold the bounds against."""
    r = lambda x: x.float().double()
    W64 = W.detach().cpu().double().reshape(W.size(0), -1)
    u, v = u.detach().cpu().double(), v.detach().cpu().double()
    if iterate:
        t = W64.t() @ u
        v = r(t / (t * t).sum().sqrt().clamp_min(eps))
        s = W64 @ v
        u = r(s / (s * s).sum().sqrt().clamp_min(eps))
    else:
        s = W64 @ v
    sigma = r(u @ s)
    return dict(v=v.float(), u=u.float(), sigma=sigma.float(), w=W64.float() / sigma.float())


def simulate_backward(sim, G):
    """dW as the kernel rounds it, from simulate()'s dict"""
    G = G.detach().cpu().float().reshape(sim["w"].shape)
    d = (G.double() * sim["w"].double()).sum().float()
    return (G - (d * sim["u"])[:, None] * sim["v"][None, :]) / sim["sigma"]
