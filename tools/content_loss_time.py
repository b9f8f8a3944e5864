"""Measurement: the content term of SynthesisLoss (losses/synthesis.py: VGG19 to relu5_1 on the prediction and on the target, the L1 of
five feature maps, and the backward pass to the prediction) for B = 16 pairs of 256 x 256 with a rand-init VGG19, on the HIP route
against the route a user has without it: torch autograd of the modules (MIOpen fp32, channels_last).

    python tools/content_loss_time.py [--pairs 16] [--size 256] [--rounds 5] [--calls 5]

One call is forward + backward: the loss and its gradient in the prediction.  The two routes alternate call by call
(_measure.alternate): after 3 warm-up calls of each, a round is CALLS calls per route and gives one median per route; the range of the
rounds' medians is reported.  The HIP route's kernels are the sums per call of their device times under torch's profiler in a run of
their own (_measure.device_events).  The routes' totals and gradients are compared with each other.  One JSON line."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd.losses import synthesis as S  # noqa: E402
from pixelsynth_amd.networks.vgg19 import VGG19  # noqa: E402
from _measure import alternate, device_events, span  # noqa: E402

# (the first name found in an event's is its kernel: k_join_pooled before k_join, bwd_prepare's kernels under "bwd")
KERNELS = ("k_input", "k_bias", "k_tap", "k_finish", "k_pool", "k_join_pooled", "k_join", "thin_in", "thin_out", "conv3x3", "f16x3", "prepare",
           "bwd", "scale")


def kernel_sums(fn, calls):
    """({kernel name: device ms per call}, every other kernel's device ms per call) of what fn launches, under torch's profiler"""
    times, other = {}, 0.0
    for name, ms in device_events(fn, calls):
        for k in KERNELS:
            if k in name:
                times[k] = times.get(k, 0.0) + ms
                break
        else:
            other += ms
    return {k: round(v / calls, 4) for k, v in times.items()}, round(other / calls, 4)


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args(argv)
    device = torch.device("cuda", 0)
    torch.manual_seed(0)
    vgg = VGG19(rand=True).to(device)
    vgg_cl = VGG19(weights=vgg.state_dict()).to(device).to(memory_format=torch.channels_last)
    gen = torch.Generator(device="cpu").manual_seed(1)
    P, H = args.pairs, args.size
    pred = torch.tanh(torch.randn(P, 3, H, H, generator=gen)).to(device).requires_grad_()
    gt = torch.tanh(torch.randn(P, 3, H, H, generator=gen)).to(device)
    pred_cl = pred.detach().contiguous(memory_format=torch.channels_last).requires_grad_()
    gt_cl = gt.contiguous(memory_format=torch.channels_last)
    if not S.hip_takes(vgg, pred, gt):
        raise SystemExit("the HIP route does not take these inputs")

    def hip():
        total, _ = S.content_loss(vgg, pred, gt)
        return total, torch.autograd.grad(total, pred)[0]

    def torch_route():
        total, _ = S.torch_content_loss(vgg_cl, pred_cl, gt_cl)
        return total, torch.autograd.grad(total, pred_cl)[0]

    routes = {"hip": hip, "torch": torch_route}
    med = alternate(routes, args.rounds, args.calls)
    (t0, g0), (t1, g1) = hip(), torch_route()
    diff = dict(total=abs(t0.item() - t1.item()) / abs(t1.item()), grad=float((g0 - g1).abs().max() / g1.abs().max()),
                grad_cosine=float(torch.nn.functional.cosine_similarity(g0.double().reshape(1, -1), g1.double().reshape(1, -1))))
    kern, other = kernel_sums(hip, args.calls)
    rec = dict(what="content_loss", pairs=P, H=H, W=H, rounds=args.rounds, calls=args.calls, kernel_ms_per_call=kern,
               other_kernels_ms_per_call=other, difference_between_routes=diff, **{f"{k}_ms_median_range": span(v) for k, v in med.items()})
    print("content term, %d pairs of %d x %d, forward + backward: HIP %.3f .. %.3f ms, torch autograd (MIOpen fp32, channels_last) "
          "%.3f .. %.3f ms; the HIP route's kernels per call %s, others %.3f ms; between the routes: total %.2e relative, gradient %.2e of "
          "its largest value, cosine %.6f" % (P, H, H, *span(med["hip"]), *span(med["torch"]), kern or "not recorded by the profiler", other,
                                              diff["total"], diff["grad"], diff["grad_cosine"]))
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
