"""Measurement: the discriminator's 4 x 4 convolutions with their backward pass (networks/disc_conv.py, csrc/disc_conv.hip) at the six
operator shapes of a training step at ndf = 64 -- both scales of the multiscale discriminator, 256 x 256 and 128 x 128.

    python tools/disc_conv_time.py [--batch 32] [--rounds 5] [--calls 5] [--shapes 0 1 2 3 4 5]

A call is the forward plus both gradients on B images.  The "f16" route (conv4x4_train: split fp16 on the matrix pipe, every layout
pass, the packing and the scaling passes included) and torch autograd of F.conv2d alternate call by call in one process between device
events (_measure.alternate): after 3 warm-up calls of each, a round is CALLS calls per route and gives one median per route; the range of
the rounds' medians is reported.  Then the "f16" route once more under torch's profiler, in a run of its own (_measure.device_events):
the device time per call of its kernels by name -- the pack, the layout passes, the products and the adding kernel, the maxima behind
the scales -- and of torch's route by the same protocol as one total.  The two routes' results are compared (largest difference over
largest value).  One JSON line per shape."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd.networks import disc_conv as DC  # noqa: E402
from _measure import alternate, device_events, span  # noqa: E402

SHAPES = [(64, 128, 129, 2), (128, 256, 65, 2), (256, 512, 33, 1), (64, 128, 65, 2), (128, 256, 33, 2), (256, 512, 17, 1)]   # (Ci, Co, H, stride)
# kernel name -> what it is (a name that contains another stands before it)
OURS = {"k_disc_conv_amax_partial": "scale: maxima", "k_disc_conv_amax_finish": "scale: finish", "k_disc_conv_pack": "pack",
        "k_disc_conv_nhwc": "layout: channels-last split", "k_disc_conv_rows": "layout: pixel-minor rows", "k_disc_conv_mfma": "product: y / grad_input",
        "k_disc_conv_gw_parts": "product: grad_weight", "k_disc_conv_gw_sum": "grad_weight: adding"}


def per_call(events, calls):
    """{kernel: [device ms per call, launches per call]} of our kernels, the device ms per call of everything else"""
    ours, rest = {}, 0.0
    for name, ms in events:
        k = next((k for k in OURS if k in name), None)
        if k is None:
            rest += ms
        else:
            ours.setdefault(k, []).append(ms)
    return {k: [round(sum(v) / calls, 4), len(v) // calls] for k, v in ours.items()}, round(rest / calls, 4)


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--shapes", type=int, nargs="+", default=list(range(len(SHAPES))))
    args = ap.parse_args(argv)
    device = torch.device("cuda", 0)
    for i in args.shapes:
        Ci, Co, H, stride = SHAPES[i]
        gen = torch.Generator().manual_seed(100 + i)
        x = F.leaky_relu(torch.randn(args.batch, Ci, H, H, generator=gen), 0.2).to(device).requires_grad_()
        w = (torch.randn(Co, Ci, 4, 4, generator=gen) / (16 * Ci) ** 0.5).to(device).requires_grad_()
        g = torch.randn(args.batch, Co, H // stride + 1, H // stride + 1, generator=gen).to(device)
        assert DC.takes(x, w, stride)

        def f16():
            y = DC.conv4x4_train(x, w, stride)
            return (y,) + torch.autograd.grad(y, (x, w), g)

        def torch_route():
            y = F.conv2d(x, w, None, stride, 2)
            return (y,) + torch.autograd.grad(y, (x, w), g)

        med = alternate({"f16": f16, "torch": torch_route}, args.rounds, args.calls)
        diffs = [float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(f16(), torch_route())]
        kern, other = per_call(device_events(f16, args.calls), args.calls)
        _, torch_ms = per_call(device_events(torch_route, args.calls), args.calls)
        ours_ms = round(sum(v[0] for v in kern.values()), 4)
        flops = 3 * 2.0 * args.batch * Co * Ci * 16 * (H // stride + 1) ** 2
        rec = dict(what="disc_conv_train", batch=args.batch, Ci=Ci, Co=Co, H=H, stride=stride, rounds=args.rounds, calls=args.calls,
                   f16_ms_median_range=span(med["f16"]), torch_ms_median_range=span(med["torch"]),
                   kernel_ms_per_call_and_launches={OURS[k] + " (" + k + ")": v for k, v in kern.items()}, f16_device_ms_per_call=ours_ms,
                   f16_other_device_ms_per_call=other, torch_device_ms_per_call=torch_ms, gflop=round(flops / 1e9, 2),
                   max_diff_over_max=dict(zip(("y", "grad_input", "grad_weight"), diffs)))
        print("%d x (%d -> %d) %d x %d stride %d: medians of %d rounds of %d calls (forward + both gradients): f16 %.3f .. %.3f ms, torch %.3f .. "
              "%.3f ms; device ms of an f16 call %.3f, of a torch call %.3f; largest difference / largest value %s"
              % (args.batch, Ci, Co, H, H, stride, args.rounds, args.calls, *span(med["f16"]), *span(med["torch"]), ours_ms, torch_ms,
                 ", ".join("%s %.1e" % kv for kv in rec["max_diff_over_max"].items())))
        for k, v in kern.items():
            print("  %-30s %-28s %9.4f ms in %d launches" % (OURS[k], k, v[0], v[1]))
        print(json.dumps(rec), flush=True)
        del x, w, g
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main(sys.argv[1:])
