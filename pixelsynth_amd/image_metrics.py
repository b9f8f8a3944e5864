"""Per-image PSNR / SSIM of image pairs on the ROCm device: the binding of ps_image_metrics (csrc/metrics.hip).

image_metrics(img1, img2, mask=None) -> (B, 6) f32 tensor, columns COLUMNS.  img1, img2 (B, C, H, W), C in {1, 3}, float32 in [0, 1] or
uint8 (converted in the kernel as x / 255, TF.to_tensor's values), any strides (NCHW or channels-last storage, read in place); mask
(B, 1, H, W), "vis" = weighted by the mask, "invis" by 1 - mask.  Without a mask the vis / invis columns are NaN.  Everything is checked
before the launch; a CPU tensor is an error (no CPU fallback).  Asynchronous on the current stream.
"""
import ctypes

import torch

from . import _lib

COLUMNS = ("psnr", "psnr_vis", "psnr_invis", "ssim", "ssim_vis", "ssim_invis")
_DTYPES = {torch.float32: 0, torch.uint8: 1}     # PS_DTYPE_F32, PS_DTYPE_U8
_MAX_B = 65535                                   # grid.y of one launch


def check_window(window_size):
    if window_size != 11:
        raise NotImplementedError("the HIP metrics kernel implements the reference's 11-tap SSIM window (window_size=11)")


def _check(img1, img2, mask):
    for name, t in (("img1", img1), ("img2", img2)):
        if not torch.is_tensor(t):
            raise TypeError(f"{name} must be a tensor")
        if t.dim() != 4:
            raise ValueError(f"{name} must be (B, C, H, W), got shape {tuple(t.shape)}")
    if img1.shape != img2.shape:
        raise ValueError(f"img1 and img2 differ in shape: {tuple(img1.shape)} vs {tuple(img2.shape)}")
    B, C, H, W = img1.shape
    if C not in (1, 3):
        raise ValueError(f"C must be 1 or 3, got {C}")
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"empty image batch {tuple(img1.shape)}")
    if img1.dtype != img2.dtype or img1.dtype not in _DTYPES:
        raise TypeError(f"img1 and img2 must both be float32 or both uint8, got {img1.dtype} and {img2.dtype}")
    if mask is not None:
        if not torch.is_tensor(mask) or tuple(mask.shape) != (B, 1, H, W):
            raise ValueError(f"mask must be (B, 1, H, W) = {(B, 1, H, W)}, got {tuple(getattr(mask, 'shape', ()))}")
        if not (mask.dtype.is_floating_point or mask.dtype == torch.bool):
            raise TypeError(f"mask must be floating point or bool, got {mask.dtype}")
    _lib.require_cuda(img1, img2, mask)
    devs = {t.device for t in (img1, img2, mask) if t is not None}
    if len(devs) != 1:
        raise ValueError(f"img1, img2 and mask must be on one device, got {sorted(map(str, devs))}")


def image_metrics(img1, img2, mask=None):
    _check(img1, img2, mask)
    B, C, H, W = img1.shape
    dev = img1.device
    if mask is not None:
        mask = mask.to(torch.float32).contiguous()
    out = torch.empty(B, 6, dtype=torch.float32, device=dev)
    strides = lambda t: (ctypes.c_int64 * 4)(*t.stride())
    with torch.cuda.device(dev):
        for b0 in range(0, B, _MAX_B):
            b1 = min(B, b0 + _MAX_B)
            a, b = img1[b0:b1], img2[b0:b1]
            m = None if mask is None else mask[b0:b1]
            nbytes = _lib.call("ps_image_metrics_workspace_bytes", b1 - b0, C, H, W)
            ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            _lib.call("ps_image_metrics", a, strides(a), b, strides(b), _DTYPES[img1.dtype], m, b1 - b0, C, H, W, out[b0:b1], ws, nbytes)
    return out
