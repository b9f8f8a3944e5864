"""PercSim of image pairs on the ROCm device: the binding of csrc/percsim.hip around the split-fp16 convolutions, for a PNet
(networks/pretrained_networks.py).

perceptual_rows(pnet, img1, img2, mask=None) -> (B, 3) f32 tensor, columns COLUMNS.  img1, img2 (B, 3, H, W), float32 in [0, 1] or
uint8 (converted in the kernel as x / 255, TF.to_tensor's values), any strides (NCHW or channels-last storage, read in place); mask
(B, 1, H, W): "vis" scores img * m, "invis" img * (1 - m), as the reference's calc_errors_quality.py does; without a mask those columns
are NaN.  The three variants share one network pass.  Everything is checked before the first launch; a CPU tensor is an error (no CPU
fallback).  H and W multiples of 256 run on the HIP path, any other size through the torch formula on the device.

A network pass: the input pass writes 2P standardised images (B, H, W, 4) (the P first are in0 of the pairs, the next P their in1);
conv1_1 (f16x3.conv3x3_thin_in, no bias), conv1_2 (act shift = -bias of conv1_1, its own bias on the way out), then per tap
ps_percsim_tap on the layer's pre-ReLU output -- the cosine partial sums and, for the first four, the max-pooled input of the next slice,
whose convolutions apply the ReLU on the way in -- and ps_percsim_finish.  Passes are cut so that one activation map stays near 1 GiB;
a pass is a guarded scope (networks.f16x3.checked).
"""
import torch

from . import _images, _lib
from .networks import f16x3
from .networks.routing import empty_nhwc

COLUMNS = ("percsim", "percsim_vis", "percsim_invis")
PLAIN, VIS, INVIS, RAW = 0, 1, 2, 3                       # PS_PERCSIM_*
_LEVELS = ((0, 1), (2, 3), (4, 5, 6), (7, 8, 9), (10, 11, 12))    # the convolutions before each tap
_MAP_BYTES = 1 << 30                                      # one activation map of a pass at most (the 64-channel maps at full size)


def pairs_per_pass(H, W):
    return max(1, min(65535, _MAP_BYTES // (2 * H * W * 64 * 4)))


def network_pass(layers, x, P, H, W):
    """The pass over x (2P, 4, H, W) channels_last (the input pass's output, or consistency.py's) with pnet.hip_layers `layers`
    -> (layers (P, 5), total (P)) f32.  At most pairs_per_pass(H, W) pairs; inside the caller's guarded scope."""
    dev, N = x.device, 2 * P
    ws, nbytes = _images.workspace("ps_percsim_workspace_bytes", P, H, W, device=dev)
    h = None
    for level, convs in enumerate(_LEVELS):
        for i in convs:
            if i == 0:
                h = f16x3.conv3x3_thin_in(x, layers["w0"])
            elif i == 1:       # conv1_1's bias enters as the act's shift: max(y + b, 0)
                h = f16x3.conv3x3(h, layers["packed"][0], f16x3.plain_relu(N, 64, dev)[0], (-layers["b0"]).expand(N, 64).contiguous())
            else:
                p = layers["packed"][i - 1]
                h = f16x3.conv3x3(h, p, *f16x3.plain_relu(N, p["Ci"], dev))
        C, Hl, Wl = h.shape[1:]
        pooled = empty_nhwc(N, C, Hl // 2, Wl // 2, h) if level < 4 else None
        _lib.call("ps_percsim_tap", h, P, H, W, level, C, pooled, ws, nbytes)
        h = pooled
    per_layer = torch.empty(P, 5, dtype=torch.float32, device=dev)
    total = torch.empty(P, dtype=torch.float32, device=dev)
    _lib.call("ps_percsim_finish", ws, nbytes, P, H, W, per_layer, total)
    return per_layer, total


def _passes(pnet, img1, img2, mask, modes):
    """Network passes over the pairs (img1, img2) in each mode of `modes` (one row block per mode) -> (total (len(modes), B),
    layers (len(modes), B, 5)), on the HIP path.  Inside the caller's guarded scope."""
    B, _, H, W = img1.shape
    dev = img1.device
    layers = pnet.hip_layers(dev)
    V = len(modes)
    per = max(1, pairs_per_pass(H, W) // V)
    total = torch.empty(V, B, dtype=torch.float32, device=dev)
    per_layer = torch.empty(V, B, 5, dtype=torch.float32, device=dev)
    for b0, b1 in _images.batches(B, per):
        n, P = b1 - b0, (b1 - b0) * V
        x = torch.empty((2 * P, H, W, 4), dtype=torch.float32, device=dev)
        a, b = img1[b0:b1], img2[b0:b1]
        m = None if mask is None else mask[b0:b1]
        for v, mode in enumerate(modes):
            _lib.call("ps_percsim_input", a, _images.strides(a), b, _images.strides(b), _images.DTYPES[img1.dtype],
                      m if mode in (VIS, INVIS) else None, mode, n, H, W, x[v * n:(v + 1) * n], x[P + v * n:P + (v + 1) * n])
        pl, tot = network_pass(layers, x.permute(0, 3, 1, 2), P, H, W)
        total[:, b0:b1] = tot.view(V, n)
        per_layer[:, b0:b1] = pl.view(V, n, 5)
    return total, per_layer


def pnet_pairs(pnet, in0, in1):
    """PNet.forward's HIP path: in0, in1 (N, 3, H, W) fp32 in [-1, 1] on the device (pnet.hip_takes) -> (total (N,), layers (N, 5)).
    A guarded scope: its fp32 rerun goes through pnet.torch_forward."""
    def run():
        if f16x3.forced_mode() == "fp32":
            tot, pl = pnet.torch_forward(in0, in1, retPerLayer=True)
            return tot, torch.stack(pl, 1)
        with torch.cuda.device(in0.device):
            tot, pl = _passes(pnet, in0, in1, None, (RAW,))
        return tot[0], pl[0]
    return f16x3.checked(in0.device, run)


def check_pnet(pnet):
    if not hasattr(pnet, "hip_takes") or not hasattr(pnet, "torch_forward"):
        raise TypeError("pnet must be a networks.pretrained_networks.PNet")


def _torch_rows(pnet, img1, img2, mask):
    """The same rows through pnet.torch_forward: the images converted with the input pass's fp32 operations, in its order."""
    a, b = ((t.float() / 255.0 if t.dtype == torch.uint8 else t) for t in (img1, img2))
    out = torch.full((a.size(0), 3), float("nan"), dtype=torch.float32, device=a.device)
    out[:, 0] = pnet.torch_forward(a * 2 - 1, b * 2 - 1)
    if mask is not None:
        for col, m in ((1, mask), (2, 1 - mask)):
            out[:, col] = pnet.torch_forward(a * m * 2 - 1, b * m * 2 - 1)
    return out


def perceptual_rows(pnet, img1, img2, mask=None):
    check_pnet(pnet)
    B, _, H, W = _images.check_images({"img1": img1, "img2": img2}, (3,), "(B, 3, H, W)")
    if mask is not None:
        _images.check_mask("mask", mask, (B, 1, H, W), _images.FLOAT_OR_BOOL)
    dev = _images.same_device(img1=img1, img2=img2, mask=mask)
    if mask is not None:
        mask = mask.to(torch.float32).contiguous()
    probe = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)   # what the HIP path takes (no data is read)
    modes = (PLAIN,) if mask is None else (PLAIN, VIS, INVIS)

    def run():
        if not pnet.hip_takes(probe, probe):
            return _torch_rows(pnet, img1, img2, mask)
        with torch.cuda.device(dev):
            total, _ = _passes(pnet, img1, img2, mask, modes)
        out = torch.full((B, 3), float("nan"), dtype=torch.float32, device=dev)
        out[:, :len(modes)] = total.t()
        return out
    with torch.no_grad():
        return f16x3.checked(dev, run)
