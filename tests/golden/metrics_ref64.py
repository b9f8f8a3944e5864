"""The quality-metric cases of tests/golden/metrics.npz and an fp64 numpy restatement of the reference's PSNR / SSIM
(evaluation/metrics.py:11-23, models/losses/ssim.py:12-67).  Shared by make_metrics_golden.py and the metric tests."""
import math

import numpy as np

from pixelsynth_amd import synthetic as syn

# name, seed, B, C, H, W, image kind (syn.metric_pair), mask kind (syn.metric_mask)
CASES = [
    ("noise_blur_256", 1, 2, 3, 256, 256, "noise_blur", "none"),
    ("noise_blur_256_ragged", 1, 2, 3, 256, 256, "noise_blur", "ragged"),
    ("noise_blur_256_fractional", 1, 2, 3, 256, 256, "noise_blur", "fractional"),
    ("noise_blur_256_empty", 1, 2, 3, 256, 256, "noise_blur", "empty"),
    ("noise_blur_256_full", 1, 2, 3, 256, 256, "noise_blur", "full"),
    ("identical_256", 2, 1, 3, 256, 256, "identical", "none"),
    ("identical_256_ragged", 2, 1, 3, 256, 256, "identical", "ragged"),
    ("flat_256", 3, 1, 3, 256, 256, "flat", "none"),
    ("flat_noise_256", 4, 1, 3, 256, 256, "flat_noise", "none"),
    ("flat_noise_256_ragged", 4, 1, 3, 256, 256, "flat_noise", "ragged"),
    ("uint8_256", 5, 2, 3, 256, 256, "uint8", "none"),
    ("uint8_256_fractional", 5, 2, 3, 256, 256, "uint8", "fractional"),
    ("odd_37x53", 6, 2, 3, 37, 53, "noise_blur", "ragged"),
    ("small_5x7", 7, 2, 3, 5, 7, "noise_blur", "fractional"),
    ("odd_255x257", 8, 1, 3, 255, 257, "noise_blur", "ragged"),
    ("c1_64x48", 9, 2, 1, 64, 48, "noise_blur", "ragged"),
    ("c1_64x48_nomask", 9, 2, 1, 64, 48, "noise_blur", "none"),
]
COLUMNS = ("psnr", "psnr_vis", "psnr_invis", "ssim", "ssim_vis", "ssim_invis")


def is_flat(name):
    return name.startswith("flat")


def case_inputs(case):
    """-> (img1, img2, mask): the images as syn.metric_pair makes them (float32 or uint8), mask (B,1,H,W) f32 or None"""
    name, seed, B, C, H, W, kind, mkind = case
    a, b = syn.metric_pair(seed, B, C, H, W, kind)
    return a, b, syn.metric_mask(mkind, seed + 100, B, H, W)


def to_unit(x):
    """uint8 -> float32 x / 255 (true division, TF.to_tensor); float32 unchanged"""
    return (x.astype(np.float32) / np.float32(255.0)).astype(np.float32) if x.dtype == np.uint8 else x


def window2d():
    """The reference's window (ssim.py:12-29): fp32 1-D taps normalised in fp32, their fp32 outer product -> (11, 11) float64."""
    g = np.array([math.exp(-((x - 5) ** 2) / float(2 * 1.5 ** 2)) for x in range(11)], np.float32)
    import torch   # torch's fp32 sum, as the reference normalises
    g = (torch.from_numpy(g) / torch.from_numpy(g).sum()).numpy()
    return (g[:, None] * g[None, :]).astype(np.float32).astype(np.float64)


def _filter(x, w):
    """depthwise 11 x 11 correlation with zero padding 5, fp64: x (B,C,H,W)"""
    B, C, H, W = x.shape
    p = np.zeros((B, C, H + 10, W + 10), np.float64)
    p[:, :, 5:5 + H, 5:5 + W] = x
    out = np.zeros((B, C, H, W), np.float64)
    for i in range(11):
        for j in range(11):
            out += w[i, j] * p[:, :, i:i + H, j:j + W]
    return out


def metrics64(img1, img2, mask=None):
    """-> (B, 6) float64 rows (COLUMNS) in fp64 with the reference's fp32 window; NaN in the masked columns without a mask."""
    a, b = to_unit(img1).astype(np.float64), to_unit(img2).astype(np.float64)
    B = a.shape[0]
    w = window2d()
    mu1, mu2 = _filter(a, w), _filter(b, w)
    s11 = _filter(a * a, w) - mu1 * mu1
    s22 = _filter(b * b, w) - mu2 * mu2
    s12 = _filter(a * b, w) - mu1 * mu2
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    smap = ((2 * mu1 * mu2 + C1) * (2 * s12 + C2)) / ((mu1 * mu1 + mu2 * mu2 + C1) * (s11 + s22 + C2))
    d2 = (a - b) ** 2
    with np.errstate(divide="ignore"):
        psnr = lambda mse: 10 * np.log10(1 / mse)
        rows = np.full((B, 6), np.nan)
        rows[:, 0] = psnr(d2.reshape(B, -1).mean(1))
        rows[:, 3] = smap.reshape(B, -1).mean(1)
        if mask is not None:
            for col, m in ((1, mask.astype(np.float64)), (2, (np.float32(1) - mask).astype(np.float64))):
                wsum = np.maximum(m.reshape(B, -1).sum(1), 1)
                rows[:, col] = psnr((d2 * m).reshape(B, -1).sum(1) / (3 * wsum))
                rows[:, col + 3] = (smap.mean(1, keepdims=True) * m).reshape(B, -1).sum(1) / wsum
    return rows
