"""FID (the Fréchet distance of Inception-v3 features, pytorch_fid's default dims = 2048) on the ROCm device: the binding of
csrc/fid.hip for a FIDInception (networks/inception.py), and the statistics.

inception_features(net, imgs) -> (B, 2048) f32 tensor.  imgs (B, 3, H, W), float32 in [0, 1] or uint8 (converted in the kernel as
x / 255, TF.to_tensor's values), any strides (NCHW or channels-last storage, read in place).  Everything is checked before the first
launch; a CPU tensor is an error (no CPU fallback).  A pass: ps_fid_input (the bilinear resize to 299 x 299 and 2 x - 1, NHWC with a
zero fourth channel), then the blocks of inception.NETWORK -- every convolution one ps_fid_conv launch with its BatchNorm folded into
weight and bias and the ReLU in the epilogue, every pool one ps_fid_pool launch, the last step of a branch writing at the branch's
channel offset of the block's output (no concat pass) -- and the mean over the 8 x 8 map.  Passes are cut so that the activations stay
near 1 GiB.  A row depends neither on its place in the batch nor on the batch's size.  If a convolution is outside what ps_fid_conv
takes (ps_fid_conv_takes, asked when the weights are packed), net.torch_forward runs on the device instead.

statistics(rows) -> (mu (D), sigma (D, D)) fp64: the mean and np.cov(rows, rowvar=False) (divisor N - 1).
frechet_distance(mu1, sigma1, mu2, sigma2) -> float: |mu1 - mu2|^2 + tr sigma1 + tr sigma2 - 2 tr sqrt(sigma1 sigma2).  The one
deliberate difference from pytorch_fid: it takes scipy's sqrtm of sigma1 sigma2 (adding 1e-6 to both diagonals when that is not finite,
dropping a small imaginary part); here the trace is the sum of the square roots of the eigenvalues of sigma1^(1/2) sigma2 sigma1^(1/2)
-- two symmetric eigh in fp64, negative eigenvalues clamped at 0, the second restricted to the range of sigma1 --, the same number where
sqrtm is well defined and defined where it is not (fewer rows than dimensions make both covariances singular).  Torch fp64 calls on the device the statistics are on: a few
GFLOP once per run."""
import numpy as np
import torch

from . import _images, _lib
from .networks import inception as I

MAX_S2, MAX_S1, AVG_S1, MEAN = 0, 1, 2, 3                 # PS_FID_*
_POOL_MODES = {"max2": MAX_S2, "max1": MAX_S1, "avg": AVG_S1}
_PASS_BYTES = 1 << 30
_IMAGE_BYTES = 4 * 147 * 147 * (32 + 64)                  # the largest pair of maps alive at once: Conv2d_2b_3x3's input and output


def images_per_pass():
    return max(1, _PASS_BYTES // _IMAGE_BYTES)


def pack_conv(w, b, stride=1, padding=(0, 0)):
    """w (Co, Ci, KH, KW), b (Co) fp32 on the device -> the layer as ps_fid_conv takes it (include/pixelsynth_fid.h: the weights in the
    order of the kernel's LDS image, Ci padded with zeros to a multiple of 4), or None when ps_fid_conv_takes says no."""
    Co, Ci, KH, KW = w.shape
    ph, pw = padding
    Cp = (Ci + 3) // 4 * 4
    if not _lib.call("ps_fid_conv_takes", KH, KW, stride, ph, pw, Cp, Co):
        return None
    T = _lib.call("ps_fid_conv_co_tile", Co)
    K, CB = KH * KW * Cp, (Co + T - 1) // T
    S = (K + 63) // 64
    w2 = torch.zeros(CB * T, S * 64, dtype=torch.float32, device=w.device)
    wk = torch.zeros(Co, KH, KW, Cp, dtype=torch.float32, device=w.device)
    wk[..., :Ci] = w.detach().float().permute(0, 2, 3, 1)
    w2[:Co, :K] = wk.reshape(Co, K)
    # (cb, t, i, s, c, kk, j) -> (cb, s, c, t, kk, i, j)
    wp = w2.view(CB, T // 16, 16, S, 4, 4, 4).permute(0, 3, 4, 1, 5, 2, 6).contiguous().view(-1)
    assert wp.numel() == _lib.call("ps_fid_conv_packed_floats", KH, KW, Cp, Co)
    return dict(wp=wp, bias=b.detach().float().contiguous(), Ci=Cp, Co=Co, KH=KH, KW=KW, stride=stride, ph=ph, pw=pw)


def _nhwc_map(x, what):
    if not (torch.is_tensor(x) and x.dim() == 4 and x.dtype == torch.float32 and x.is_contiguous()):
        raise ValueError(f"{what} must be a contiguous float32 (N, H, W, C) tensor")
    _lib.require_cuda(x)


def _out(out, coff, shape, C, dev):
    """The output map of a launch: a new (N, Ho, Wo, C) one, or `out` checked against the launch"""
    if out is None:
        return torch.empty(shape + (C,), dtype=torch.float32, device=dev), 0
    _nhwc_map(out, "out")
    if tuple(out.shape[:3]) != shape or coff < 0 or coff + C > out.size(3) or out.device != dev:
        raise ValueError(f"out {tuple(out.shape)} on {out.device} does not hold channels {coff} .. {coff + C - 1} of a {shape} map on {dev}")
    return out, coff


def conv_shape(layer, H, W):
    return ((H + 2 * layer["ph"] - layer["KH"]) // layer["stride"] + 1, (W + 2 * layer["pw"] - layer["KW"]) // layer["stride"] + 1)


def conv(x, layer, out=None, coff=0):
    """max(conv(x) + bias, 0) of a pack_conv layer on x (N, H, W, >= Ci) -> channels coff .. coff + Co - 1 of out (a new (N, Ho, Wo, Co)
    map without one); the other channels of out are not touched."""
    _nhwc_map(x, "x")
    N, H, W, ldx = x.shape
    Ho, Wo = conv_shape(layer, H, W)
    if ldx < layer["Ci"] or Ho < 1 or Wo < 1:
        raise ValueError(f"x {tuple(x.shape)} does not fit a {layer['KH']} x {layer['KW']} convolution of {layer['Ci']} channels")
    out, coff = _out(out, coff, (N, Ho, Wo), layer["Co"], x.device)
    _lib.call("ps_fid_conv", x, ldx, layer["wp"], layer["wp"].numel(), layer["bias"], N, H, W, layer["Ci"], layer["KH"], layer["KW"],
              layer["stride"], layer["ph"], layer["pw"], layer["Co"], out, out.size(3), coff)
    return out


def pool_shape(mode, H, W):
    return (1, 1) if mode == MEAN else ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if mode == MAX_S2 else (H, W)


def pool(x, mode, out=None, coff=0):
    """The pool `mode` (MAX_S2, MAX_S1, AVG_S1, MEAN) of x (N, H, W, C) -> channels coff .. coff + C - 1 of out, as conv writes."""
    _nhwc_map(x, "x")
    N, H, W, C = x.shape
    if mode == MAX_S2 and (H < 3 or W < 3):
        raise ValueError(f"x {tuple(x.shape)} is too small for a 3 x 3 pool")
    out, coff = _out(out, coff, (N,) + pool_shape(mode, H, W), C, x.device)
    _lib.call("ps_fid_pool", x, C, mode, N, H, W, C, out, out.size(3), coff)
    return out


def input_pass(imgs):
    """imgs (B, 3, H, W) float32 in [0, 1] or uint8, any strides -> (B, 299, 299, 4): resized, 2 x - 1, channel 3 zero"""
    B, _, H, W = imgs.shape
    out = torch.empty((B, I.SIZE, I.SIZE, 4), dtype=torch.float32, device=imgs.device)
    _lib.call("ps_fid_input", imgs, _images.strides(imgs), _images.DTYPES[imgs.dtype], B, H, W, out)
    return out


def _step_shape(layers, step, H, W, C):
    if isinstance(step, tuple):
        shapes = [_step_shape(layers, s, H, W, C) for s in step]
        return shapes[0][:2] + (sum(s[2] for s in shapes),)
    if step in I.POOLS:
        return pool_shape(_POOL_MODES[step], H, W) + (C,)
    return conv_shape(layers[step], H, W) + (layers[step]["Co"],)


def _network(layers, x):
    """x (N, 299, 299, 4), the input pass's output -> (N, 2048)"""
    N = x.size(0)
    for _, branches in I.NETWORK:
        shapes = []
        for steps in branches:
            s = tuple(x.shape[1:])
            for step in steps:
                s = _step_shape(layers, step, *s)
            shapes.append(s)
        assert len({s[:2] for s in shapes}) == 1, shapes
        out = torch.empty((N,) + shapes[0][:2] + (sum(s[2] for s in shapes),), dtype=torch.float32, device=x.device)
        off = 0
        for steps, shape in zip(branches, shapes):
            h = x
            for k, step in enumerate(steps):
                dst = (out, off) if k == len(steps) - 1 else (None, 0)
                if isinstance(step, tuple):          # both on the same input, side by side (the last step of its branch)
                    conv(h, layers[step[0]], out, off)
                    conv(h, layers[step[1]], out, off + layers[step[0]]["Co"])
                elif step in I.POOLS:
                    h = pool(h, _POOL_MODES[step], *dst)
                else:
                    h = conv(h, layers[step], *dst)
            off += shape[2]
        x = out
    return pool(x, MEAN).view(N, -1)


def inception_features(net, imgs):
    if not hasattr(net, "hip_layers") or not hasattr(net, "torch_forward"):
        raise TypeError("net must be a networks.inception.FIDInception")
    B = _images.check_images({"imgs": imgs}, (3,), "(B, 3, H, W)")[0]
    dev = _images.same_device(imgs=imgs)
    if next(net.parameters()).device != dev:
        raise ValueError(f"imgs are on {dev}, the network on {next(net.parameters()).device}")
    with torch.no_grad(), torch.cuda.device(dev):
        layers = net.hip_layers(dev)
        rows = []
        for b0, b1 in _images.batches(B, images_per_pass()):
            part = imgs[b0:b1]
            if layers is None:
                rows.append(net.torch_forward(part.float() / 255.0 if part.dtype == torch.uint8 else part))
            else:
                rows.append(_network(layers, input_pass(part)))
        return rows[0] if len(rows) == 1 else torch.cat(rows)


# ---- the statistics
def _f64(a):
    return a.detach().double() if torch.is_tensor(a) else torch.from_numpy(np.asarray(a, dtype=np.float64))


def statistics(rows):
    """rows (N, D), N >= 2 (a tensor or an array) -> (mu (D), sigma (D, D)) fp64 tensors on the rows' device"""
    rows = _f64(rows)
    if rows.dim() != 2 or rows.size(0) < 2:
        raise ValueError(f"rows must be (N, D) with N >= 2, got shape {tuple(rows.shape)}")
    mu = rows.mean(0)
    d = rows - mu
    return mu, d.t() @ d / (rows.size(0) - 1)


def _sym_eig(m):
    w, v = torch.linalg.eigh((m + m.t()) * 0.5)
    return w.clamp_min(0.0), v


def frechet_distance(mu1, sigma1, mu2, sigma2):
    mu1, sigma1, mu2, sigma2 = (_f64(a) for a in (mu1, sigma1, mu2, sigma2))
    D = mu1.numel()
    if mu1.dim() != 1 or mu2.shape != mu1.shape or tuple(sigma1.shape) != (D, D) or tuple(sigma2.shape) != (D, D):
        raise ValueError(f"mu (D) and sigma (D, D) of one D expected, got {tuple(mu1.shape)}, {tuple(sigma1.shape)}, "
                         f"{tuple(mu2.shape)}, {tuple(sigma2.shape)}")
    # sigma1^(1/2) = V sqrt(w) V^T.  With A = V sqrt(w) over the eigenvalues that are not numerically zero, A^T sigma2 A has the
    # non-zero eigenvalues of sigma1^(1/2) sigma2 sigma1^(1/2): the null space of a singular sigma1 (rounding noise whose square
    # roots would add up) never enters.
    w, v = _sym_eig(sigma1)
    keep = w > w.max() * D * torch.finfo(torch.float64).eps
    a = v[:, keep] * w[keep].sqrt()
    ev, _ = _sym_eig(a.t() @ sigma2 @ a)
    diff = mu1 - mu2
    return float(diff @ diff + torch.trace(sigma1) + torch.trace(sigma2) - 2.0 * ev.sqrt().sum())


def fid_of_rows(rows1, rows2):
    """FID of two sets of feature rows."""
    return frechet_distance(*statistics(rows1), *statistics(rows2))
