"""Per-image PSNR / SSIM of image pairs on the ROCm device: the binding of ps_image_metrics (csrc/metrics.hip).

image_metrics(img1, img2, mask=None) -> (B, 6) f32 tensor, columns COLUMNS.  img1, img2 (B, C, H, W), C in {1, 3}, float32 in [0, 1] or
uint8 (converted in the kernel as x / 255, TF.to_tensor's values), any strides (NCHW or channels-last storage, read in place); mask
(B, 1, H, W), "vis" = weighted by the mask, "invis" by 1 - mask.  Without a mask the vis / invis columns are NaN.  Everything is checked
before the launch; a CPU tensor is an error (no CPU fallback).  Asynchronous on the current stream.
"""
import torch

from . import _images, _lib

COLUMNS = ("psnr", "psnr_vis", "psnr_invis", "ssim", "ssim_vis", "ssim_invis")


def check_window(window_size):
    if window_size != 11:
        raise NotImplementedError("the HIP metrics kernel implements the reference's 11-tap SSIM window (window_size=11)")


def image_metrics(img1, img2, mask=None):
    B, C, H, W = _images.check_images({"img1": img1, "img2": img2}, (1, 3), "(B, C, H, W)")
    if mask is not None:
        _images.check_mask("mask", mask, (B, 1, H, W), _images.FLOAT_OR_BOOL)
    dev = _images.same_device(img1=img1, img2=img2, mask=mask)
    if mask is not None:
        mask = mask.to(torch.float32).contiguous()
    out = torch.empty(B, 6, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        for b0, b1 in _images.batches(B):
            a, b = img1[b0:b1], img2[b0:b1]
            m = None if mask is None else mask[b0:b1]
            ws, nbytes = _images.workspace("ps_image_metrics_workspace_bytes", b1 - b0, C, H, W, device=dev)
            _lib.call("ps_image_metrics", a, _images.strides(a), b, _images.strides(b), _images.DTYPES[img1.dtype], m, b1 - b0, C, H, W,
                      out[b0:b1], ws, nbytes)
    return out
