"""PercSim of 128 uint8 pairs at 256 x 256 on the HIP path (csrc/percsim.hip around the split-fp16 convolutions) against the same PNet
through torch (networks.f16x3.decoder_conv("fp32"): MIOpen fp32 convolutions), unmasked and masked (three variants per pair), timed with
CUDA events after warm-up.  Prints one JSON line per case: ms per batch of each path, fp32-equivalent GFLOP per pair from the shapes, the
fraction of the fp32 (157.3 TFLOP/s) and fp16 (2.5 PFLOP/s) dense peaks, and how far the two paths' results are apart.

    python tools/percsim_time.py [--pairs 128] [--reps 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd import synthetic as syn  # noqa: E402
from pixelsynth_amd.networks import f16x3  # noqa: E402
from pixelsynth_amd.networks.pretrained_networks import PNet  # noqa: E402
from pixelsynth_amd.perceptual import perceptual_rows  # noqa: E402

PEAK_FP32, PEAK_FP16 = 157.3e12, 2.5e15


def gflop_per_image(H, W):
    """2 x MACs of VGG16's 13 convolutions up to relu5_3 at H x W"""
    cfg = [(3, 64), (64, 64), "M", (64, 128), (128, 128), "M", (128, 256), (256, 256), (256, 256), "M", (256, 512), (512, 512),
           (512, 512), "M", (512, 512), (512, 512), (512, 512)]
    tot, h, w = 0, H, W
    for c in cfg:
        if c == "M":
            h, w = h // 2, w // 2
        else:
            tot += 2 * 9 * c[0] * c[1] * h * w
    return tot / 1e9


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        out = fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / reps, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=128)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--hip-only", action="store_true", help="only the HIP path (for a kernel trace)")
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    net = PNet(use_gpu=True, weights={k: torch.from_numpy(v) for k, v in syn.vgg16_state_dict(7).items()})
    a, b = syn.metric_pair(1, args.pairs, 3, 256, 256, "uint8")
    m = syn.metric_mask("ragged", 2, args.pairs, 256, 256)
    a, b, m = (torch.from_numpy(x).to(dev) for x in (a, b, m))
    for masked in (False, True):
        mm = m if masked else None
        variants = 3 if masked else 1
        t_hip, r_hip = timed(lambda: perceptual_rows(net, a, b, mm), args.reps)
        gf = 2 * variants * gflop_per_image(256, 256)
        res = {"pairs": args.pairs, "masked": masked, "hip_ms": round(t_hip, 3), "gflop_per_pair": round(gf, 2),
               "hip_tflops": round(gf * args.pairs / t_hip, 1), "hip_frac_fp32_peak": round(gf * args.pairs / t_hip * 1e12 / PEAK_FP32, 3),
               "hip_frac_fp16_peak": round(gf * args.pairs / t_hip * 1e12 / PEAK_FP16, 3)}
        if not args.hip_only:
            with f16x3.decoder_conv("fp32"):
                t_ref, r_ref = timed(lambda: perceptual_rows(net, a, b, mm), max(1, args.reps // 2))
            d = (r_hip[:, :variants].double() - r_ref[:, :variants].double()).abs()
            res.update(torch_fp32_ms=round(t_ref, 3), speedup=round(t_ref / t_hip, 2), torch_tflops=round(gf * args.pairs / t_ref, 1),
                       max_abs_diff=float("%.3g" % float(d.max())), max_rel_diff=float("%.3g" % float((d / r_ref[:, :variants].double().abs()).max())))
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
