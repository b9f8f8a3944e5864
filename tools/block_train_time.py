"""Measurement: the 1 x 1 projection and the resample-and-sum of the refinement decoder's four resampling blocks in training mode
(csrc/block_train.hip through networks/block_train.py) at their own shapes -- 64 -> 128 Down on 256^2, 128 -> 256 Down on 128^2,
256 -> 128 Up on 64^2, 128 -> 128 Up on 128^2 -- for B = 16 frames, against the route they take without the opt-in: F.conv2d, and
_resample of each branch and their sum, under torch autograd on the same channels-last tensors.

    python tools/block_train_time.py [--frames 16] [--rounds 5] [--calls 5] [--shapes 0,1,2,3]

Row (a), the 1 x 1 convolution: forward plus the gradients in x, weight and bias for one grad_output.  Row (b), the join: forward plus the
gradient in both operands.  The two routes alternate call by call (_measure.alternate): after 3 warm-up calls of each, a round is CALLS
calls per route and gives one median per route; the range of the rounds' medians is reported.  The HIP route's kernels are the medians of
their device times under torch's profiler in a run of their own (_measure.device_events, kernel_medians).  The routes' gradients are
compared with each other and, for the join, the first frame of each with torch autograd of the same resampling on the host.  One JSON
line per shape and row."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd import _lib  # noqa: E402
from pixelsynth_amd.networks import architectures as A, block_train as BT  # noqa: E402
from _measure import alternate, device_events, kernel_medians, span  # noqa: E402

SHAPES = ((64, 128, "Down", 256), (128, 256, "Down", 128), (256, 128, "Up", 64), (128, 128, "Up", 128))      # (Ci, Co, join, H = W of the block's input)
# (the _bwd names before their forward twins: the first name found in an event's is its kernel)
KERNELS = ("k_grad_weight", "k_sum_parts", "k_conv1x1", "k_upsample_add_bwd", "k_pool_add_bwd", "k_upsample_add", "k_pool_add")


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

    def rand(*shape):
        return torch.randn(*shape, generator=gen).to(device)

    for Ci, Co, kind, H in (SHAPES[int(i)] for i in args.shapes.split(",")):
        W = H
        # (a) the projection, on the block's input
        x = rand(B, Ci, H, W).contiguous(memory_format=cl).requires_grad_()
        w = (rand(Co, Ci, 1, 1) * Ci ** -0.5).contiguous(memory_format=cl).requires_grad_()
        b = rand(Co).requires_grad_()
        g = rand(B, Co, H, W).contiguous(memory_format=cl)
        conv = {"hip": lambda: torch.autograd.grad(BT.conv1x1_train(x, w, b), (x, w, b), g),
                "torch": lambda: torch.autograd.grad(F.conv2d(x, w, b), (x, w, b), g)}
        med = alternate(conv, args.rounds, args.calls)
        ours, ref = conv["hip"](), conv["torch"]()
        diff = {k: float((p - q).abs().max() / q.abs().max()) for k, p, q in zip(("dx", "dw", "db"), ours, ref)}
        kern = kernel_medians(device_events(conv["hip"], args.calls), KERNELS)
        rec = dict(what="conv1x1_train", Ci=Ci, Co=Co, frames=B, H=H, W=W, rounds=args.rounds, calls=args.calls,
                   parts=_lib.call("ps_conv1x1_grad_weight_parts", B * H * W, Ci, Co), kernel_ms_median=kern, max_diff_over_max=diff,
                   **{f"{k}_ms_median_range": span(v) for k, v in med.items()})
        print("(a) 1 x 1, %d -> %d, %d frames of %d x %d, forward + three gradients: HIP %.3f .. %.3f ms, torch autograd %.3f .. %.3f ms; "
              "kernels %s; largest differences / largest value: dx %.2e, dw %.2e, db %.2e"
              % (Ci, Co, B, H, W, *span(med["hip"]), *span(med["torch"]), kern or "not recorded by the profiler", diff["dx"], diff["dw"], diff["db"]))
        print(json.dumps(rec), flush=True)
        del x, g, ours, ref
        # (b) the join, on the two branches' outputs (Co channels at the block's input size)
        a = rand(B, Co, H, W).contiguous(memory_format=cl).requires_grad_()
        c = rand(B, Co, H, W).contiguous(memory_format=cl).requires_grad_()
        side = 2 * H if kind == "Up" else H // 2
        g = rand(B, Co, side, side).contiguous(memory_format=cl)
        join = {"hip": lambda: torch.autograd.grad(BT.resample_sum_train(kind, a, c), (a, c), g),
                "torch": lambda: torch.autograd.grad(A._resample(kind, a) + A._resample(kind, c), (a, c), g)}
        med = alternate(join, args.rounds, args.calls)
        ours, ref = join["hip"](), join["torch"]()
        diff = float((ours[0] - ref[0]).abs().max() / ref[0].abs().max())
        # ... and each route's first frame against torch autograd of the same resampling on the host
        host = torch.zeros(1, Co, H, W, requires_grad=True)
        (A._resample(kind, host) * g[:1].cpu().contiguous()).sum().backward()
        vs_host = {k: float((r[0][:1].cpu() - host.grad).abs().max() / host.grad.abs().max()) for k, r in (("hip", ours), ("torch", ref))}
        kern = kernel_medians(device_events(join["hip"], args.calls), KERNELS)
        rec = dict(what="resample_sum_train", kind=kind, C=Co, frames=B, H=H, W=W, rounds=args.rounds, calls=args.calls, kernel_ms_median=kern,
                   max_diff_over_max=diff, max_diff_to_host_over_max=vs_host, **{f"{k}_ms_median_range": span(v) for k, v in med.items()})
        print("(b) join %s, %d channels, %d frames of %d x %d, forward + backward: HIP %.3f .. %.3f ms, torch autograd %.3f .. %.3f ms; "
              "kernels %s; largest difference / largest value between the routes %.2e, of the first frame to torch autograd on the host: HIP %.2e, torch %.2e"
              % (kind, Co, B, H, W, *span(med["hip"]), *span(med["torch"]), kern or "not recorded by the profiler", diff, vs_host["hip"],
                 vs_host["torch"]))
        print(json.dumps(rec), flush=True)
        del a, c, g, ours, ref


if __name__ == "__main__":
    main(sys.argv[1:])
