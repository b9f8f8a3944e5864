"""What the tests of the depth Unet's training kernels (csrc/unet_train.hip, networks/unet_train.py) compare against: the fp64 formulas
of include/pixelsynth_unet_train.h, the mirror of its split into parts, an fp64 twin of Unet.forward whose ReLU decisions can be frozen,
and the bounds.  The statistics' and y's forms are tests/_norm_train_ref.py's (imported, with its u = 2^-24).

Bounds beyond that file's.

  z        y's bound and one more rounding (slope * y), u |z|.
  running  With m the momentum, keep = fl(1 - m), m32 = fl(m), f = N / (N - 1), f32 = fl(f), every product and sum of
             running_mean' = fl(fl(running_mean * keep) + fl(mean32 * m32))
             running_var'  = fl(fl(running_var * keep) + fl(fl(var32 * f32) * m32))
           is one rounding on the kernel's own fp32 mean32 / var32, themselves within (u |mean64|, bv) of the fp64 statistics (bv:
           stat_bounds).  First order, against the fp64 update of the same stored value:
             mean   |running_mean| (1 - m) 2 u  (keep, product)  +  m |mean64| 3 u  (mean32, m32, product)  +  u |result|  (sum)
             var    |running_var| (1 - m) 2 u  +  m f (bv + 4 u var64)  (var32; f32, m32, two products)  +  u |result|
           times 1.01 for the second-order terms.  num_batches_tracked is an integer: exact.
  up       out = sum of four products w * relu(x), the weights exact and every term >= 0.  A term passes through its product's rounding
           and through at most three sums', four roundings: 4 u sum |w relu(x)|, 1.01 in front for the second-order terms.
  adjoint  the weight w = w_row * w_col is exact; a term passes through its product's rounding and through at most k - 1 sums' (the first
           sum, onto 0, is exact), k = (rows heard from) * (columns heard from) <= 16 the gathered terms: 1.01 k u sum |w g|.
  g        every gradient: |g - g64| <= 4 max(E32, 1e-6 max |g64|), E32 the error of torch's fp32 autograd of the same formula on the
           host (grad_bound of _norm_train_ref).  Elements within KINK = 1e-4 of a kink (y = 0, a = 0, b = 0) are left out of the dx /
           da / db comparisons alone; at most KINK_SHARE = 1e-3 of the elements may be (randn inputs: about 8e-5).
"""
import torch
import torch.nn.functional as F

from _norm_train_ref import U, check, forward64, forward_bound, grad_bound, stat_bounds, stats64  # noqa: F401

MAX_PARTS, PART_ROWS, MAX_C = 256, 256, 65536       # PS_UNET_TRAIN_* of the header (tests/test_unet_train_cpu.py holds them to it)
THREADS, MAX_CW = 256, 64
KINK, KINK_SHARE = 1e-4, 1e-3
SLOPE = 0.2


# ---- the plan ----------------------------------------------------------------------------------------------------------------------------
def part_rows(N):
    return PART_ROWS * -(-(-(-N // PART_ROWS)) // MAX_PARTS)


def plan(N, C):
    """(rows per part, parts, channel quads of a workgroup, its row lanes, workgroups across the channels)"""
    rows, cw = part_rows(N), min(C // 4, MAX_CW)
    return rows, -(-N // rows), cw, THREADS // cw, -(-(C // 4) // cw)


def workspace_bytes(N, C):
    up = lambda n: (n + 255) // 256 * 256
    return up(plan(N, C)[1] * 2 * C * 8) + up(2 * C * 4)


# (B, H, W, C): the issue's shapes, then one on each side of every boundary of the plan -- one part | two (N = 256 | 257), one chunk of
# channels | two (C = 256 | 260), parts of 256 rows | of 512 (N = 65536 | 65537: 256 parts | 129), every lane with a row | lanes without
# (cw = 1: 256 lanes, N = 2), threads left over (cw = 3: 85 lanes, one idle thread)
BN_SHAPES = [(1, 1, 2, 4), (2, 1, 1, 8), (1, 2, 2, 256), (3, 5, 7, 12), (2, 16, 16, 32),
             (1, 16, 16, 4), (1, 1, 257, 4), (1, 2, 2, 260), (1, 256, 256, 4), (1, 1, 65537, 4)]
# (B, H, W) x (Ca, Cb): the issue's, then both sides of the one boundary of the launch plan -- outputs in one workgroup of 256 float4s |
# in two ((1, 8, 8) x (4, none) is 256, (1, 8, 8) x (4, 4) is 512; (1, 3, 11) x (4, 4) is 264: a second workgroup of 8 live threads)
UP_SHAPES = [(1, 1, 1), (1, 1, 2), (1, 2, 1), (2, 3, 5), (1, 8, 8), (3, 16, 16), (1, 3, 11)]
UP_CHANNELS = [(4, None), (4, 4), (8, 12), (32, 32)]
UP_WIDE = ((1, 2, 2), (256, 256))


def bn_inputs(B, H, W, C, seed=0, offset=0.3, spread=1.5):
    gen = torch.Generator().manual_seed(seed)
    x = offset + spread * torch.randn(B, C, H, W, generator=gen)
    weight, bias = 1 + 0.3 * torch.randn(C, generator=gen), 0.3 * torch.randn(C, generator=gen)
    dy, dz = torch.randn(B, C, H, W, generator=gen), torch.randn(B, C, H, W, generator=gen)
    return x, weight, bias, dy, dz


# ---- the batch norm ----------------------------------------------------------------------------------------------------------------------
def bn_forward64(x, weight, bias, eps, slope=None):
    """_norm_train_ref.forward64 with the shared weight and bias, and z -> dict(mean, var, m2, scale, shift, y, z)"""
    f = forward64(x, weight.reshape(1, -1), bias.reshape(1, -1), eps, False)
    f["z"] = None if slope is None else torch.where(f["y"] > 0, f["y"], slope * f["y"])
    return f


def bn_backward64(x, dy, dz, weight, bias, eps, slope):
    """The header's backward formulas in fp64 -> dx, dweight, dbias; dy or dz may be None"""
    f = bn_forward64(x, weight, bias, eps)
    x, w = x.double(), weight.double().view(1, -1, 1, 1)
    g = torch.zeros_like(x)
    if dy is not None:
        g = g + dy.double()
    if dz is not None:
        g = g + dz.double() * torch.where(f["y"] > 0, torch.ones_like(x), torch.full_like(x, float(slope)))
    rstd = torch.rsqrt(f["var"] + eps).view(1, -1, 1, 1)
    xhat = (x - f["mean"].view(1, -1, 1, 1)) * rstd
    dbias, dweight = g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))
    n = x.numel() // x.size(1)
    k1, k2 = (w * dbias.view(1, -1, 1, 1)) / n, (w * dweight.view(1, -1, 1, 1)) / n
    return rstd * (w * g - k1 - xhat * k2), dweight, dbias


def bn_autograd(x, weight, bias, dy, dz, eps, slope, dtype):
    """(dx, dweight, dbias) of torch's own batch norm + leaky ReLU by autograd in `dtype` on the host"""
    x, weight, bias = (t.detach().to(dtype).clone().requires_grad_() for t in (x, weight, bias))
    y = F.batch_norm(x, None, None, weight, bias, True, 0.1, eps)
    loss = 0
    if dy is not None:
        loss = loss + (y * dy.to(dtype)).sum()
    if dz is not None:
        loss = loss + (F.leaky_relu(y, slope) * dz.to(dtype)).sum()
    loss.backward()
    return x.grad, weight.grad, bias.grad


def z_bound(x, f):
    return forward_bound(x, f) + U * f["z"].abs()


def running64(running_mean, running_var, x, momentum):
    """The fp64 update of the stored values on x's fp64 statistics -> (mean', var', mean's bound, var's bound): the docstring"""
    m, var, _ = stats64(x)
    n = x.numel() // x.size(1)
    f = n / (n - 1)
    rm, rv = running_mean.double().cpu(), running_var.double().cpu()
    rm2, rv2 = rm * (1 - momentum) + m * momentum, rv * (1 - momentum) + var * f * momentum
    bv = stat_bounds(x, rows=n)[1]
    bm = 1.01 * U * (2 * rm.abs() * (1 - momentum) + 3 * momentum * m.abs() + rm2.abs())
    bvv = 1.01 * (U * (2 * rv.abs() * (1 - momentum) + rv2.abs()) + momentum * f * (bv + 4 * U * var))
    return rm2, rv2, bm, bvv


def kink_free(values):
    """The elements further than KINK from the kink at 0 -> (mask, the share left out)"""
    keep = values.double().abs() > KINK
    return keep, 1.0 - keep.double().mean().item()


# ---- relu -> bilinear x2 of a concatenation ----------------------------------------------------------------------------------------------
def up_matrix(n):
    """(2 n, n) fp64: row d holds the weights of output index d on the inputs, by the header's rule; exact quarters"""
    M = torch.zeros(2 * n, n, dtype=torch.float64)
    for d in range(2 * n):
        s = max((d + 0.5) / 2 - 0.5, 0.0)
        i0 = int(s)
        i1, w = min(i0 + 1, n - 1), s - int(s)
        M[d, i0] += 1 - w
        M[d, i1] += w
    return M


def up_cat(a, b):
    return a if b is None else torch.cat((a, b), 1)


def up_forward64(a, b):
    """-> (out, sum |w relu(x)|), the same thing here: every term is >= 0"""
    h = up_cat(a, b).double().clamp_min(0)
    out = torch.einsum("ph,bchw,qw->bcpq", up_matrix(h.size(2)), h, up_matrix(h.size(3)))
    return out, out


def up_adjoint64(g, src, c0):
    """grad of the operand src whose channels start at c0 of g -> (grad, sum |w g|, k the terms gathered per pixel)"""
    H, W = src.shape[2:]
    My, Mx = up_matrix(H), up_matrix(W)
    gs = g.double()[:, c0:c0 + src.size(1)]
    mask = (src > 0).double()
    grad = torch.einsum("ph,bcpq,qw->bchw", My, gs, Mx) * mask
    mag = torch.einsum("ph,bcpq,qw->bchw", My, gs.abs(), Mx) * mask
    k = ((My > 0).sum(0).view(-1, 1) * (Mx > 0).sum(0).view(1, -1)).double()
    return grad, mag, k


def up_autograd(a, b, g, dtype):
    """(da, db) of F.interpolate(F.relu(cat)) by torch autograd in `dtype` on the host"""
    a = a.detach().to(dtype).clone().requires_grad_()
    b = None if b is None else b.detach().to(dtype).clone().requires_grad_()
    out = F.interpolate(F.relu(up_cat(a, b)), scale_factor=2, mode="bilinear", align_corners=False)
    (out * g.to(dtype)).sum().backward()
    return a.grad, None if b is None else b.grad


# ---- the network's twin ------------------------------------------------------------------------------------------------------------------
class Decisions:
    """The sign decisions of one forward in call order: record() appends what a run decided, replay() hands them out again and counts
    the elements where the twin's own sign differs"""

    def __init__(self):
        self.masks, self.at, self.differ, self.total = [], 0, 0, 0

    def record(self, t):
        self.masks.append((t > 0).cpu())

    def replay(self, t):
        mask = self.masks[self.at]
        self.at += 1
        self.differ += int((mask != (t > 0)).sum())
        self.total += mask.numel()
        return mask


def twin_forward(net, x, frozen=None):
    """Unet.forward's expressions on the host in net's precision, its modules called as they are (the spectral norm's hook, the norms'
    running update); with `frozen` (Decisions of another run, in this order: the seven leaky ReLUs, then the eight ReLUs) each
    activation takes that run's decisions instead of its own signs"""
    def leaky(h):
        return F.leaky_relu(h, SLOPE) if frozen is None else torch.where(frozen.replay(h), h, SLOPE * h)

    def relu(h):
        return F.relu(h) if frozen is None else torch.where(frozen.replay(h), h, torch.zeros_like(h))
    skips, h = [], x
    for i in range(8):
        h = getattr(net, f"conv{i + 1}")(h if i == 0 else leaky(h))
        if net._ENC_NORM[i]:
            h = getattr(net, net._ENC_NORM[i])(h)
        skips.append(h)
    for i in range(8):
        h = F.interpolate(relu(h), scale_factor=2, mode="bilinear", align_corners=False)
        h = getattr(net, f"dconv{i + 1}")(h)
        if net._DEC_NORM[i]:
            h = torch.cat((getattr(net, net._DEC_NORM[i])(h), skips[6 - i]), 1)
    return h
