"""Time the quality-metric kernel (csrc/metrics.hip) on 128 image pairs of 256 x 256 with a mask, fp32 and uint8, next to the
reference's formula in torch (five depthwise 11 x 11 F.conv2d per pair, models/losses/ssim.py:33-67, plus the PSNR of
evaluation/metrics.py) on the same GPU, and check both give the same numbers.

    python tools/metrics_time.py [--pairs 128] [--size 256] [--iters 50]

Prints microseconds per batch (_measure.looped_ms: one pair of device events around ITERS calls, after 5 warm-up calls) and, for the kernel, the fraction of two lower bounds from the shapes:
bytes / 8 TB/s and fp32-equivalent flops / 157.3 TFLOP/s (MI355X_MICROARCH.md; the kernel runs its filters in fp64, which this
chip issues at the fp32 vector rate without packing)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from pixelsynth_amd import synthetic as syn  # noqa: E402
from pixelsynth_amd.image_metrics import image_metrics  # noqa: E402
from _measure import looped_ms  # noqa: E402

HBM = 8.0e12
FP32 = 157.3e12


def torch_formula(a, b, m, window):
    """the reference's PSNR / SSIM in torch fp32 (vis only): (B, 4) psnr, psnr_vis, ssim, ssim_vis"""
    C = a.shape[1]
    conv = lambda x: F.conv2d(x, window, padding=5, groups=C)
    mu1, mu2 = conv(a), conv(b)
    s11, s22, s12 = conv(a * a) - mu1 * mu1, conv(b * b) - mu2 * mu2, conv(a * b) - mu1 * mu2
    smap = ((2 * mu1 * mu2 + 1e-4) * (2 * s12 + 9e-4)) / ((mu1 * mu1 + mu2 * mu2 + 1e-4) * (s11 + s22 + 9e-4))
    B = a.shape[0]
    d2 = (a - b).pow(2)
    psnr = 10 * (1 / d2.view(B, -1).mean(1)).log10()
    psnr_v = 10 * (1 / ((d2 * m).view(B, -1).sum(1) / (3 * m.view(B, -1).sum(1).clamp(min=1)))).log10()
    ssim = smap.view(B, -1).mean(1)
    ssim_v = (smap.mean(1, keepdim=True) * m).view(B, -1).sum(1) / m.view(B, -1).sum(1).clamp(min=1)
    return torch.stack([psnr, psnr_v, ssim, ssim_v], 1)


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    B, C, S = args.pairs, 3, args.size
    h8 = [torch.from_numpy(x) for x in syn.metric_pair(1, B, C, S, S, "uint8")]
    a8, b8 = (x.to(dev) for x in h8)
    a, b = (x.float().div(255).to(dev) for x in h8)     # on the host, as TF.to_tensor (the device may multiply by 1/255 instead)
    m = torch.from_numpy(syn.metric_mask("fractional", 2, B, S, S)).to(dev)
    g = torch.tensor([__import__("math").exp(-((x - 5) ** 2) / 4.5) for x in range(11)], dtype=torch.float32)
    g = g / g.sum()
    window = (g[:, None] @ g[None, :]).expand(C, 1, 11, 11).contiguous().to(dev)

    px = B * S * S
    bytes_f32 = px * C * 4 * 2 + px * 4
    bytes_u8 = px * C * 2 + px * 4
    # fp32-equivalent flops of the formula: 5 maps x 11 taps x 2 passes x 2 flops + 3 products + ~20 for the map and the sums
    flops = px * C * (5 * 11 * 2 * 2 + 3 + 20)
    t_f32 = looped_ms(lambda: image_metrics(a, b, m), args.iters, 5) * 1e3
    t_u8 = looped_ms(lambda: image_metrics(a8, b8, m), args.iters, 5) * 1e3
    t_torch = looped_ms(lambda: torch_formula(a, b, m, window), args.iters, 5) * 1e3
    ours = image_metrics(a, b, m)[:, [0, 1, 3, 4]]
    ref = torch_formula(a, b, m, window)
    dp = (ours[:, :2] - ref[:, :2]).abs().max().item()
    ds = (ours[:, 2:] - ref[:, 2:]).abs().max().item()
    assert dp < 1e-3 and ds < 1e-4, (dp, ds)
    assert torch.equal(image_metrics(a8, b8, m), image_metrics(a, b, m))
    bound = lambda nbytes: max(nbytes / HBM, flops / FP32) * 1e6
    res = {
        "pairs": B, "size": S, "channels": C, "mask": True,
        "kernel_f32_us": round(t_f32, 2), "kernel_u8_us": round(t_u8, 2), "torch_formula_f32_us": round(t_torch, 2),
        "bound_bytes_f32_us": round(bytes_f32 / HBM * 1e6, 2), "bound_bytes_u8_us": round(bytes_u8 / HBM * 1e6, 2),
        "bound_flops_fp32_us": round(flops / FP32 * 1e6, 2),
        "kernel_f32_fraction_of_bound": round(bound(bytes_f32) / t_f32, 3),
        "kernel_u8_fraction_of_bound": round(bound(bytes_u8) / t_u8, 3),
        "torch_formula_fraction_of_bound": round(bound(bytes_f32) / t_torch, 3),
        "speedup_vs_torch_f32": round(t_torch / t_f32, 2),
        "max_diff_vs_torch": {"psnr_db": dp, "ssim": ds},
    }
    print(json.dumps(res))


if __name__ == "__main__":
    main()
