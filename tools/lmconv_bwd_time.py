"""Measurement: the backward pass of one locally masked convolution (csrc/lmconv_bwd.hip through lmconv_backward) at the PixelCNN's
four layer shapes -- 513 -> 80, 160 -> 80, 160 -> 160, and 80 -> 80 with dilation 2 -- for B = 16 frames of the 32 x 32 code grid,
against torch autograd through the reference's unfold formula (F.unfold, the mask product, matmul) on the device.

    python tools/lmconv_bwd_time.py [--frames 16] [--rounds 5] [--calls 10]

Both routes compute grad_input, grad_weight and grad_bias for the same grad_output; the forward passes (and torch's graph) are made
outside the timed part.  The two routes alternate call by call (_measure.alternate): after 3 warm-up calls of each, a round is CALLS
calls per route and gives one median per route; the range of the rounds' medians is reported, with the HIP route's two halves
(grad_input alone; grad_weight and grad_bias alone) beside it, and the largest differences between the two routes' results.  One JSON
line per shape."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd.lmconv.locally_masked_convolution import lmconv_backward  # noqa: E402
from _measure import alternate, span  # noqa: E402

H = W = 32
SHAPES = ((513, 80, 1), (160, 80, 1), (160, 160, 1), (80, 80, 2))


def unfold_lmconv(x, m, w, b, dilation):
    """The reference's forward (models/lmconv/locally_masked_convolution.py:25-43) with one mask copy per image"""
    B, Ci = x.shape[:2]
    xu = F.unfold(x, (3, 3), dilation=dilation, padding=dilation)
    xm = (xu.view(B, Ci, 9, -1) * m.unsqueeze(1)).view(B, Ci * 9, -1)
    return (w.view(w.size(0), -1).matmul(xm) + b.view(1, -1, 1)).view(B, -1, x.size(2), x.size(3))


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args(argv)
    device = torch.device("cuda", 0)
    B = args.frames
    gen = torch.Generator(device="cpu").manual_seed(0)
    for Ci, Co, dil in SHAPES:
        x = torch.randn(B, Ci, H, W, generator=gen).to(device).requires_grad_()
        w = (torch.randn(Co, Ci, 3, 3, generator=gen) * 0.05).to(device).requires_grad_()
        b = torch.randn(Co, generator=gen).to(device).requires_grad_()
        m = (torch.rand(B, 9, H * W, generator=gen) < 0.5).float().to(device)
        g = torch.randn(B, Co, H, W, generator=gen).to(device)
        y = unfold_lmconv(x, m, w, b, dil)
        xd, wd = x.detach(), w.detach()
        routes = {"hip": lambda: lmconv_backward(g, xd, m, wd, dil, True, True, True),
                  "torch": lambda: torch.autograd.grad(y, (x, w, b), g, retain_graph=True),
                  "hip_grad_input": lambda: lmconv_backward(g, xd, m, wd, dil, True, False, False),
                  "hip_grad_weight_bias": lambda: lmconv_backward(g, xd, m, wd, dil, False, True, True)}
        med = alternate(routes, args.rounds, args.calls)
        ours, ref = routes["hip"](), routes["torch"]()
        diff = {k: float((p - q).abs().max()) for k, p, q in zip(("grad_input", "grad_weight", "grad_bias"), ours, ref)}
        flops = 2.0 * 9 * Ci * Co * B * H * W                       # of each of the two products
        rec = dict(what="lmconv_backward", Ci=Ci, Co=Co, dilation=dil, frames=B, H=H, W=W, rounds=args.rounds, calls=args.calls,
                   flop_per_product=flops, max_abs_diff=diff, **{f"{k}_ms_median_range": span(v) for k, v in med.items()})
        print("lmconv backward %d -> %d, dilation %d, %d frames of %d x %d: medians of %d rounds of %d calls: HIP %.3f .. %.3f ms "
              "(grad_input %.3f .. %.3f, grad_weight + grad_bias %.3f .. %.3f), torch autograd of the unfold formula %.3f .. %.3f ms; "
              "largest differences: input %.3g, weight %.3g, bias %.3g"
              % (Ci, Co, dil, B, H, W, args.rounds, args.calls, *span(med["hip"]), *span(med["hip_grad_input"]),
                 *span(med["hip_grad_weight_bias"]), *span(med["torch"]), diff["grad_input"], diff["grad_weight"], diff["grad_bias"]))
        print(json.dumps(rec), flush=True)
        del y


if __name__ == "__main__":
    main(sys.argv[1:])
