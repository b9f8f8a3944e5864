"""What the tests of the PixelCNN's training kernels (csrc/pixelcnn_train.hip, lmconv/train_ops.py) compare against: the fp64 formulas of
include/pixelsynth_pixelcnn_train.h, its constants, and the bounds.

Bounds.  u = 2^-24 bounds the relative error of one fp32 rounding; C = channels; r = rstd64, c = x - mean64, xh = c r.

  mean     K + S1 / C in fp64, rounded once; the fp64 sum of C differences errs by at most C 2^-53 of sum |x - K| <= 2 C max |x|:
                                                                            |mean - mean64| <= u |mean64| + C^2 2^-52 max |x|
  rstd     var = (S2 - S1^2 / C) / (C - 1) about K, one of the samples: S2 <= C sum (x - mean)^2 (the header), so the fp64 subtraction
           loses a factor C at the worst and each of S2, S1^2 / C is known to C 2^-53 of itself: the fp64 var is off by at most
           T_VAR = C^2 2^-50 of itself (a factor 4 of room; 6e-12 at C = 80).  rstd = (var + eps)^-1/2 in fp64, rounded ONCE:
                                                                            |rstd - rstd64| <= rstd64 (u + T_VAR / 2) (1 + 2^-10)
           (the last factor: the second-order terms).  var itself is not an output; a negative or zero one would show here, on
           100 + 0.01 randn above all, where an fp32 sum of squares about 0 has no correct digit left.
  xh       the four rounded steps from the fp64 statistics: mean's rounding u |mean| r, the subtraction's u |c| r, rstd's
           (u + T_VAR / 2) |xh|, the product's u |xh|; |c| <= |x| + |mean|, |xh| <= (|x| + |mean|) r:
                                                                            E_xh = (4 u (|x| + |mean|) r + T_VAR / 2 |xh|) (1 + 2^-10)
  z        = xh + skip: + u |z| where there is a skip; without PONO xh = x is exact.
  y        elu is 1-Lipschitz and continuous with a continuous derivative, so an element whose z changes sign between the kernel and fp64
           is covered: |y - y64| <= E_z + C_ELU u |y64|, the last term expm1f's own error (measured, below); the same for elu(-z).
  out      = u + xh s, s = sigmoid(g) <= 1 with a relative error C_SIG u (measured, below): E_xh s + (C_SIG + 1) u |xh s| + u |out|.
  C_ELU, C_SIG   not guessed: the largest error of torch's own fp32 F.elu / torch.sigmoid on the host against fp64, in units of
           u |value|, over the inputs the tests draw (transcendental_ratios below; 0.3 + 1.5 randn and the +-30 case); the constant is
           the smallest power of two at or above twice that, as C_GRAD of test_lmconv_bwd_gpu.py was set.  Measured: elu 0.997, sigmoid
           1.93 (docs/LAB_NOTEBOOK.md has the run).
  g        the project's rule for gradients: |g - g64| <= 4 max(E32, 1e-6 max |g64|), E32 the largest error of torch's fp32 evaluation
           of the same formula on the host (grad_bound).  No element is left out of any comparison: nothing here has a kink.
  grad_logits   the same rule against fp64 autograd of F.cross_entropy; rows outside the group are +0 bit for bit.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
EPS = 1e-5
WIDE_LOCATIONS, MAX_CHANNELS = 262144, 65536       # PS_PCT_* of the header (tests/test_pixelcnn_train_cpu.py holds them to it)
C_ELU, C_SIG = 2, 4                               # measured ratios 0.997 and 1.93 (the docstring)
SLACK = 1 + 2.0 ** -10


def t_var(C):
    return C * C * 2.0 ** -50


def inputs(B, C, H, W, seed=0, scale=None):
    """x, skip, u = 0.3 + 1.5 randn, randn, randn; dy (B,2C,H,W) = randn.  scale "offset": x = 100 + 0.01 randn; "large": every
    operand +-30 with random signs"""
    gen = torch.Generator().manual_seed(seed)
    x = 0.3 + 1.5 * torch.randn(B, C, H, W, generator=gen)
    skip, u = torch.randn(B, C, H, W, generator=gen), torch.randn(B, C, H, W, generator=gen)
    dy = torch.randn(B, 2 * C, H, W, generator=gen)
    if scale == "offset":
        x = 100 + 0.01 * torch.randn(B, C, H, W, generator=gen)
    elif scale == "large":
        x, skip = (30.0 * torch.sign(torch.randn(B, C, H, W, generator=gen)) for _ in range(2))
        x = x + torch.randn(B, C, H, W, generator=gen)
    return x, skip, u, dy


def pono64(x):
    """-> mean, rstd (B,1,H,W), xh, all fp64, of the fp32 x: the reference's PONO (unbiased variance, eps inside the root)"""
    x = x.double()
    var, mean = torch.var_mean(x, dim=1, keepdim=True, unbiased=True)
    rstd = (var + EPS).rsqrt()
    return mean, rstd, (x - mean) * rstd


def chained_mean(x):
    """The mean as the header orders its additions, on the host in fp64 and rounded once: K = channel 0, four chains (chain k: the
    channels k, k + 4, ... ascending) of x - K, joined as (s0 + s1) + (s2 + s3), mean = K + S1 / C.  Every step is one IEEE operation,
    so the kernel's mean has to be these BITS whatever lanes it ran on -- on inputs where another order of the additions gives
    another fp32 value (order_sensitive), that is a test of the order itself"""
    v = x.double().numpy()
    K = v[:, 0]
    chains = []
    for k in range(4):
        acc = 0.0 * K
        for c in range(k, v.shape[1], 4):
            acc = acc + (v[:, c] - K)
        chains.append(acc)
    S1 = (chains[0] + chains[1]) + (chains[2] + chains[3])
    return torch.from_numpy(K + S1 / v.shape[1]).float().unsqueeze(1)


def order_sensitive(B, C, H, W, seed=0):
    """randn with +-2^60 in channel 1 and its negative in channel 5 (one chain: they cancel exactly there, and swallow the values
    between them in a sum that runs over the channels in sequence), and the same at channels 6 and 14"""
    assert C >= 15
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(B, C, H, W, generator=gen)
    big = 2.0 ** 60 * torch.sign(torch.randn(B, H, W, generator=gen))
    x[:, 1], x[:, 5], x[:, 6], x[:, 14] = big, -big, -big, big
    return x


def elu_slope(t):
    return torch.where(t > 0, torch.ones_like(t), t.exp())


def norm_act_forward64(x, skip=None, norm=True, act="celu"):
    """-> dict(mean, rstd, xh, z, y) in fp64"""
    mean, rstd, xh = pono64(x) if norm else (None, None, x.double())
    z = xh if skip is None else xh + skip.double()
    y = z if act is None else F.elu(z) if act == "elu" else torch.cat([F.elu(z), F.elu(-z)], 1)
    return dict(mean=mean, rstd=rstd, xh=xh, z=z, y=y)


def pono_adjoint64(dz, xh, rstd):
    """dx = rstd (dz - mean_c(dz) - xh sum_c(dz xh) / (C - 1))"""
    C = dz.shape[1]
    return rstd * (dz - dz.mean(1, keepdim=True) - xh * (dz * xh).sum(1, keepdim=True) / (C - 1))


def norm_act_backward64(x, skip, dy, norm=True, act="celu"):
    """The header's backward in closed form, fp64 -> (dx, dskip)"""
    f = norm_act_forward64(x, skip, norm, act)
    z, dy, C = f["z"], dy.double(), x.shape[1]
    dz = dy if act is None else dy * elu_slope(z) if act == "elu" else dy[:, :C] * elu_slope(z) - dy[:, C:] * elu_slope(-z)
    return (pono_adjoint64(dz, f["xh"], f["rstd"]) if norm else dz), (None if skip is None else dz)


def gate_forward64(vg, u):
    C = u.shape[1]
    mean, rstd, vh = pono64(vg[:, :C])
    s = torch.sigmoid(vg[:, C:].double())
    return dict(mean=mean, rstd=rstd, vh=vh, s=s, out=u.double() + vh * s)


def gate_backward64(vg, dout):
    """-> the gradient of the whole (B,2C,H,W) operand in closed form, fp64 (u's is dout itself)"""
    C = vg.shape[1] // 2
    mean, rstd, vh = pono64(vg[:, :C])
    s, dout = torch.sigmoid(vg[:, C:].double()), dout.double()
    return torch.cat([pono_adjoint64(dout * s, vh, rstd), dout * vh * s * (1 - s)], 1)


def code_nll_backward64(logits, targets, region, group, temperature, grad_out=1.0):
    """logits (F,512,L) -> grad_out (softmax(logits / T) - onehot) / T / count on the group's locations, 0 elsewhere, fp64; targets are
    valid codes here"""
    p = torch.softmax(logits.double() / temperature, 1)
    p = p - F.one_hot(targets.long(), logits.shape[1]).movedim(-1, 1)
    take = group_mask(region, group, targets)
    return torch.where(take[:, None], p * (grad_out / temperature / take.sum().item()), torch.zeros_like(p))


def group_mask(region, group, like):
    sampled = torch.zeros_like(like, dtype=torch.bool) if region is None else region != 0
    return torch.ones_like(sampled) if group == "all" else sampled if group == "sampled" else ~sampled


def autograd(fn, tensors, dy, dtype):
    """Gradients of sum(fn(*tensors) * dy) by torch autograd in `dtype` on the host (None stays None)"""
    leaves = [None if t is None else t.detach().cpu().to(dtype).clone().requires_grad_() for t in tensors]
    (fn(*leaves) * dy.cpu().to(dtype)).sum().backward()
    return [None if t is None else t.grad for t in leaves]


# ---------------------------------------------------------------------------------------------------------------------- the bounds
def stat_bounds(x, f):
    C = x.shape[1]
    return (U * f["mean"].abs() + C * C * 2.0 ** -52 * x.double().abs().amax(1, keepdim=True),
            f["rstd"] * (U + t_var(C) / 2) * SLACK)


def xh_bound(x, f):
    C = x.shape[1]
    return (4 * U * (x.double().abs() + f["mean"].abs()) * f["rstd"] + t_var(C) / 2 * f["xh"].abs()) * SLACK


def y_bound(x, skip, norm, act, f):
    ez = xh_bound(x, f) if norm else torch.zeros_like(f["z"])
    if skip is not None:
        ez = ez + U * f["z"].abs() * SLACK
    if act is None:
        return ez
    return (torch.cat([ez, ez], 1) if act == "celu" else ez) + C_ELU * U * f["y"].abs()


def out_bound(vg, f):
    C = vg.shape[1] // 2
    fx = dict(mean=f["mean"], rstd=f["rstd"], xh=f["vh"])
    prod = (f["vh"] * f["s"]).abs()
    return (xh_bound(vg[:, :C], fx) * f["s"] + (C_SIG + 1) * U * prod + U * f["out"].abs()) * SLACK


def transcendental_ratios(seed=0):
    """(elu, sigmoid): the largest |fp32 - fp64| / (u |fp64|) of torch's own fp32 F.elu / torch.sigmoid on the host over the values
    the tests draw (inputs(): the plain and the +-30 case, both signs)"""
    worst = [0.0, 0.0]
    for scale in (None, "large"):
        x, skip, _, _ = inputs(4, 80, 8, 8, seed, scale)
        z = torch.cat([x, -x, skip, x + skip]).flatten()
        for k, fn in enumerate((F.elu, torch.sigmoid)):
            want = fn(z.double())
            ok = want.abs() > 1e-300
            worst[k] = max(worst[k], ((fn(z).double() - want).abs()[ok] / (U * want.abs()[ok])).max().item())
    return tuple(worst)


def grad_bound(g32, g64):
    """-> (bound, E32)"""
    E32 = (g32.double() - g64).abs().max().item()
    return 4 * max(E32, 1e-6 * g64.abs().max().item()), E32


def check(name, got, want, bound):
    """max |got - want| / bound, printed and returned; bound a number or a tensor of want's shape"""
    got = got.detach()
    err = (got.double().cpu() - want).abs()
    bound = torch.as_tensor(bound, dtype=torch.float64).expand_as(err)
    assert got.shape == want.shape and torch.isfinite(got).all(), name
    ratio = (err / bound.clamp_min(1e-300)).max().item()
    print(f"{name}: max |err| {err.max().item():.3e}, error / bound {ratio:.3f}")
    return ratio
