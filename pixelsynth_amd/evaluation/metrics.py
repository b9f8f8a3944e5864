"""Mirror of the reference's evaluation/metrics.py: psnr and ssim_metric on the HIP kernel (csrc/metrics.hip), perceptual_sim as
there.  Images in [0, 1]; mask (B, 1, H, W) or None.  Each returns (B,)."""
from ..image_metrics import image_metrics
from ..losses.ssim import ssim


def ssim_metric(img1, img2, mask=None):
    """metrics.py:6-7"""
    return ssim(img1, img2, mask=mask, size_average=False)


def psnr(img1, img2, mask=None):
    """metrics.py:11-23: 10 log10(1 / mse); masked, mse = sum(d^2 m) / (3 max(sum m, 1)).  Not clamped (identical images: inf)."""
    return image_metrics(img1, img2, mask)[:, 0 if mask is None else 1]


def perceptual_sim(img1, img2, vgg16):
    """metrics.py:27-31: the caller's network (the reference's PNet) on the images mapped to [-1, 1]; nothing of it is built here."""
    return vgg16(img1 * 2 - 1, img2 * 2 - 1)
