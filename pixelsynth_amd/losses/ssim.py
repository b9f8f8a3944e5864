"""Mirror of the reference's models/losses/ssim.py (ssim, SSIM): the SSIM of image pairs, forward only, on the HIP kernel
(csrc/metrics.hip).  Same signatures and the same results, including the reference's quirk that a MASKED call returns the per-image
vector even with size_average=True (ssim.py:61-67).  Only the 11-tap window the reference uses is implemented."""
import torch

from ..image_metrics import check_window, image_metrics


def _ssim(img1, img2, mask, size_average):
    rows = image_metrics(img1, img2, mask)
    if mask is not None:
        return rows[:, 4]
    return rows[:, 3].mean() if size_average else rows[:, 3]


def ssim(img1, img2, window_size=11, mask=None, size_average=True):
    """ssim.py:112-124.  img1, img2 (B, C, H, W) in [0, 1] (float32, or uint8 read as x / 255); mask (B, 1, H, W) or None.
    -> scalar (size_average, no mask) or (B,)."""
    check_window(window_size)
    return _ssim(img1, img2, mask, size_average)


class SSIM(torch.nn.Module):
    """ssim.py:82-109."""

    def __init__(self, window_size=11, size_average=True):
        super().__init__()
        check_window(window_size)
        self.window_size = window_size
        self.size_average = size_average

    def forward(self, img1, img2, mask=None):
        return _ssim(img1, img2, mask, self.size_average)
