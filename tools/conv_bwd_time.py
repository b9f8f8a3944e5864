"""Measurement: the backward pass of the split-fp16 3 x 3 convolution (csrc/conv_bwd.hip through networks/f16x3.py:conv3x3_train) at the
refinement decoder's layer shapes -- 64 -> 64 and 128 -> 128 at 256 x 256, 128 -> 256 and 256 -> 256 at 128 x 128, 256 -> 256 and
256 -> 128 at 64 x 64 -- for B = 16 frames, against torch autograd of F.conv2d (MIOpen fp32, channels_last) on the same tensors.

    python tools/conv_bwd_time.py [--frames 16] [--rounds 5] [--calls 5] [--shapes 0,1,2,3,4,5]

Both routes compute grad_input, grad_weight and grad_bias for the same grad_output; the forward passes (and the graphs) are made outside
the timed part.  The two routes alternate call by call (_measure.alternate): after 3 warm-up calls of each, a round is CALLS calls per
route and gives one median per route; the range of the rounds' medians is reported.  The HIP route's steps are timed the same way as
calls of their own -- prepare (max |g|, grad_bias, g * s), grad_input (the forward kernel on the scaled g with the flipped weight, its
packing included; the unscale pass), grad_weight (GEMM and adding kernel in one call) -- and its kernels as the medians of their device
times under torch's profiler in a run of their own (_measure.device_events, kernel_medians), which is what separates the GEMM from the
adding kernel.  One JSON line per shape."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd import _lib  # noqa: E402
from pixelsynth_amd.networks import f16x3  # noqa: E402
from _measure import alternate, device_events, kernel_medians, span  # noqa: E402

SHAPES = ((256, 64, 64), (256, 128, 128), (128, 128, 256), (128, 256, 256), (64, 256, 256), (64, 256, 128))      # (H = W, Ci, Co)
KERNELS = ("k_prep_partial", "k_prep_finish", "k_scale", "k_grad_weight_parts", "k_grad_weight_sum", "k_conv3x3_f16x3", "k_pack")


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(map(str, range(len(SHAPES)))))
    args = ap.parse_args(argv)
    device = torch.device("cuda", 0)
    B = args.frames
    gen = torch.Generator(device="cpu").manual_seed(0)
    cl = torch.channels_last
    for H, Ci, Co in (SHAPES[int(i)] for i in args.shapes.split(",")):
        W = H
        x = torch.relu(torch.randn(B, Ci, H, W, generator=gen) * 1.5).to(device).contiguous(memory_format=cl).requires_grad_()
        w = (torch.randn(Co, Ci, 3, 3, generator=gen) / (3 * Ci ** 0.5)).to(device).contiguous(memory_format=cl).requires_grad_()
        b = torch.randn(Co, generator=gen).to(device).requires_grad_()
        g = (torch.randn(B, Co, H, W, generator=gen) * 1e-3).to(device).contiguous(memory_format=cl)
        y_hip = f16x3.conv3x3_train(x, w, b)
        y_torch = F.conv2d(x, w, b, 1, 1)
        # the HIP route's steps as calls of their own, on buffers of their own
        ws = torch.empty(_lib.call("ps_conv3x3_bwd_workspace_bytes", B, H, W, Ci, Co), dtype=torch.uint8, device=device)
        gs, scale2, gb = torch.empty_like(g), torch.empty(2, device=device), torch.empty(Co, device=device)
        gw = torch.empty(Co, 3, 3, Ci, device=device)
        flag = torch.zeros(1, dtype=torch.int32, device=device)
        xd, wd = x.detach(), w.detach()
        prepare = lambda: _lib.call("ps_conv3x3_bwd_prepare_f32", g, B, H, W, Co, gs, scale2, gb, ws, ws.numel())
        prepare()
        gx = [None]

        def conv():
            gx[0] = f16x3.conv3x3(gs, f16x3.pack3x3(wd.flip(2, 3).transpose(0, 1), check=False), overflow=flag)
        conv()
        routes = {"hip": lambda: torch.autograd.grad(y_hip, (x, w, b), g, retain_graph=True),
                  "torch": lambda: torch.autograd.grad(y_torch, (x, w, b), g, retain_graph=True),
                  "hip_prepare": prepare,
                  "hip_grad_input_conv": conv,
                  "hip_grad_input_unscale": lambda: _lib.call("ps_conv3x3_bwd_unscale_f32", gx[0], gx[0].numel(), scale2),
                  "hip_grad_weight": lambda: _lib.call("ps_conv3x3_grad_weight_f16x3", xd, gs, scale2, B, H, W, Ci, Co, gw, flag, ws, ws.numel())}
        med = alternate(routes, args.rounds, args.calls)
        ours, ref = routes["hip"](), routes["torch"]()
        diff = {k: float((p - q).abs().max() / q.abs().max()) for k, p, q in zip(("grad_input", "grad_weight", "grad_bias"), ours, ref)}
        kern = kernel_medians(device_events(routes["hip"], args.calls), KERNELS)
        flops = 2.0 * 9 * Ci * Co * B * H * W                       # of each of the two products (a third of what the split multiplies)
        rec = dict(what="conv3x3_backward", Ci=Ci, Co=Co, frames=B, H=H, W=W, rounds=args.rounds, calls=args.calls,
                   parts=_lib.call("ps_conv3x3_bwd_parts", B, H, W, Ci, Co), workspace_bytes=ws.numel(), flop_per_product=flops,
                   kernel_ms_median=kern, max_diff_over_max=diff, overflow=int(flag.item()),
                   **{f"{k}_ms_median_range": span(v) for k, v in med.items()})
        print("conv3x3 backward %d -> %d, %d frames of %d x %d: medians of %d rounds of %d calls: HIP %.3f .. %.3f ms (prepare %.3f .. %.3f; "
              "grad_input: convolution %.3f .. %.3f, unscale %.3f .. %.3f; grad_weight %.3f .. %.3f), torch autograd of F.conv2d %.3f .. %.3f "
              "ms; kernels %s; largest differences / largest value: input %.2e, weight %.2e, bias %.2e"
              % (Ci, Co, B, H, W, args.rounds, args.calls, *span(med["hip"]), *span(med["hip_prepare"]), *span(med["hip_grad_input_conv"]),
                 *span(med["hip_grad_input_unscale"]), *span(med["hip_grad_weight"]), *span(med["torch"]),
                 kern or "not recorded by the profiler", diff["grad_input"], diff["grad_weight"], diff["grad_bias"]))
        print(json.dumps(rec), flush=True)
        del y_hip, y_torch


if __name__ == "__main__":
    main(sys.argv[1:])
