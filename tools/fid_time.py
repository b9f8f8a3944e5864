"""Inception-v3 features (FID, dims = 2048) of 128 uint8 images at 256 x 256 resident on the device: the HIP path (csrc/fid.hip,
fid.inception_features) against the same FIDInception through torch (FIDInception.torch_forward: the library's fp32 convolutions).
Every shape is warmed first (2 calls), the two paths alternate inside one call, each run between two device events on a synchronised
device (_measure.event_ms).  Prints one JSON line: ms per batch of each path (the median and the spread over the repetitions), their ratio, GFLOP per
image from the shapes, the fraction of the fp32 dense peak (157.3 TFLOP/s), and how far the two paths' features are apart.  With
--table also one JSON line per distinct convolution shape at that batch: the ps_fid_conv launch against torch's conv2d + relu on the
same operands (NCHW, as torch_forward runs it), and how often the network runs the shape.

    python tools/fid_time.py [--images 128] [--reps 7] [--table] [--hip-only]
"""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd import fid, synthetic as syn  # noqa: E402
from pixelsynth_amd.networks.inception import FIDInception, conv_shapes  # noqa: E402
from _measure import event_ms  # noqa: E402

PEAK_FP32 = 157.3e12


def gflop_per_image():
    """2 x MACs of the 94 convolutions at 299 x 299 (the unpadded channel counts)"""
    return sum(2 * kh * kw * ci * co * ((H + 2 * ph - kh) // s + 1) * ((W + 2 * pw - kw) // s + 1)
               for _, kh, kw, s, ph, pw, ci, co, H, W in conv_shapes()) / 1e9


def take_turns(fns, reps, warm=2):
    """-> ([sorted ms per repetition] per function, the last outputs): every function warmed, then run in turn `reps` times, each run
    timed by _measure.event_ms"""
    for fn in fns:
        for _ in range(warm):
            fn()
    ms, outs = [[] for _ in fns], [None] * len(fns)
    for _ in range(reps):
        for k, fn in enumerate(fns):
            ms[k].append(event_ms(lambda: outs.__setitem__(k, fn())))
    return [sorted(m) for m in ms], outs


def stats(ms):
    return {"median": round(ms[len(ms) // 2], 3), "min": round(ms[0], 3), "max": round(ms[-1], 3)}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=128)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--table", action="store_true", help="also time every distinct convolution shape")
    ap.add_argument("--hip-only", action="store_true", help="only the HIP path (for a kernel trace)")
    args = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    net = FIDInception(weights={k: torch.from_numpy(v) for k, v in syn.inception_state_dict(11).items()}, use_gpu=True)
    imgs = torch.from_numpy(syn.metric_pair(1, args.images, 3, 256, 256, "uint8")[1]).to(dev)
    hip = lambda: fid.inception_features(net, imgs)
    if args.hip_only:
        (ms,), _ = take_turns([hip], args.reps)
        print(json.dumps({"images": args.images, "hip_ms": stats(ms)}), flush=True)
        return
    with torch.no_grad():
        ref = lambda: net.torch_forward(imgs.float() / 255.0)
        (ms_hip, ms_ref), (r_hip, r_ref) = take_turns([hip, ref], args.reps)
    gf = gflop_per_image()
    t_hip, t_ref = ms_hip[len(ms_hip) // 2], ms_ref[len(ms_ref) // 2]
    d = (r_hip.double() - r_ref.double()).abs()
    print(json.dumps({"images": args.images, "size": 256, "hip_ms": stats(ms_hip), "torch_fp32_ms": stats(ms_ref),
                      "torch_over_hip": round(t_ref / t_hip, 3), "gflop_per_image": round(gf, 3),
                      "hip_tflops": round(gf * args.images / t_hip, 1), "torch_tflops": round(gf * args.images / t_ref, 1),
                      "hip_frac_fp32_peak": round(gf * args.images / t_hip * 1e12 / PEAK_FP32, 3),
                      "max_abs_diff": float("%.3g" % float(d.max())), "feature_max": float("%.3g" % float(r_ref.max()))}), flush=True)
    if not args.table:
        return
    count = {}
    for _, *shape in conv_shapes():
        count[tuple(shape)] = count.get(tuple(shape), 0) + 1
    g = torch.Generator().manual_seed(3)
    N = args.images
    for (kh, kw, s, ph, pw, ci, co, H, W), times in count.items():
        cp = (ci + 3) // 4 * 4
        x = torch.randn(N, H, W, cp, generator=g).to(dev)
        w = (torch.randn(co, cp, kh, kw, generator=g) * (2.0 / (kh * kw * ci)) ** 0.5).to(dev)
        b = torch.zeros(co, device=dev)
        layer = fid.pack_conv(w, b, s, (ph, pw))
        xc = x.permute(0, 3, 1, 2).contiguous()
        (m_hip, m_ref), _ = take_turns([lambda: fid.conv(x, layer), lambda: F.relu(F.conv2d(xc, w, b, s, (ph, pw)))], max(3, args.reps // 2))
        gfl = 2 * kh * kw * ci * co * ((H + 2 * ph - kh) // s + 1) * ((W + 2 * pw - kw) // s + 1) * N / 1e9
        a, r = m_hip[len(m_hip) // 2], m_ref[len(m_ref) // 2]
        print(json.dumps({"conv": f"{kh}x{kw} s{s} p({ph},{pw}) {ci}->{co} @ {H}x{W}", "runs": times, "hip_ms": round(a, 3),
                          "torch_ms": round(r, 3), "torch_over_hip": round(r / a, 2), "hip_tflops": round(gfl / a, 1),
                          "torch_tflops": round(gfl / r, 1)}), flush=True)
        del x, w, xc, layer


if __name__ == "__main__":
    main()
