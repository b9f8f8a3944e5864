"""Measurement: the refinement decoder's four thin layers in training mode (csrc/thin_train.hip through networks/thin_train.py) at their own
shapes -- block 0's 3 x 3 and 1 x 1 from 4 to 64 channels, block 7's from 128 to 3 -- for B = 16 frames of 256 x 256, against the route
they take without the opt-in: torch autograd of F.conv2d on the same channels-last tensors.

    python tools/thin_train_time.py [--frames 16] [--size 256] [--rounds 5] [--calls 5] [--layers 0,1,2,3]

Per layer: forward plus the gradients in x, weight and bias for one grad_output.  The two routes alternate call by call
(_measure.alternate): after 3 warm-up calls of each, a round is CALLS calls per route and gives one median per route; the range of the
rounds' medians is reported.  The HIP route's kernels are the medians of their device times under torch's profiler in a run of their own
(_measure.device_events, kernel_medians).  The routes' gradients are compared with each other.  One JSON line per layer."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd import _lib  # noqa: E402
from pixelsynth_amd.networks import thin_train as TT  # noqa: E402
from _measure import alternate, device_events, kernel_medians, span  # noqa: E402

LAYERS = (("in", 4, 64, 3), ("in", 4, 64, 1), ("out", 128, 3, 3), ("out", 128, 3, 1))      # (kind, Ci, Co, k)
KERNELS = ("k_thin_grad_weight", "k_thin_sum_parts", "k_thin_expand", "k_thin_add_bias", "k_thin_in", "k_thin_out", "k_conv1x1")


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--layers", default=",".join(map(str, range(len(LAYERS)))))
    args = ap.parse_args(argv)
    device = torch.device("cuda", 0)
    B, H, W = args.frames, args.size, args.size
    gen = torch.Generator(device="cpu").manual_seed(0)
    cl = torch.channels_last

    def rand(*shape):
        return torch.randn(*shape, generator=gen).to(device)

    for kind, Ci, Co, k in (LAYERS[int(i)] for i in args.layers.split(",")):
        x = rand(B, Ci, H, W).contiguous(memory_format=cl).requires_grad_()
        w = (rand(Co, Ci, k, k) * (Ci * k * k) ** -0.5).contiguous(memory_format=cl).requires_grad_()
        b = rand(Co).requires_grad_()
        g = rand(B, Co, H, W).contiguous(memory_format=cl)
        fn = TT.conv_thin_in_train if kind == "in" else TT.conv_thin_out_train
        routes = {"hip": lambda: torch.autograd.grad(fn(x, w, b), (x, w, b), g),
                  "torch": lambda: torch.autograd.grad(F.conv2d(x, w, b, padding=k // 2), (x, w, b), g)}
        med = alternate(routes, args.rounds, args.calls)
        ours, ref = routes["hip"](), routes["torch"]()
        diff = {n: float((p - q).abs().max() / q.abs().max()) for n, p, q in zip(("dx", "dw", "db"), ours, ref)}
        kern = kernel_medians(device_events(routes["hip"], args.calls), KERNELS)
        wide, T = (Co, Ci) if kind == "in" else (Ci, Co)
        rec = dict(what="conv_thin_%s_train" % kind, Ci=Ci, Co=Co, k=k, frames=B, H=H, W=W, rounds=args.rounds, calls=args.calls,
                   parts=_lib.call("ps_thin_train_parts", B, H, W, wide, T, k), kernel_ms_median=kern, max_diff_over_max=diff,
                   **{f"{n}_ms_median_range": span(v) for n, v in med.items()})
        print("%d x %d, %d -> %d, %d frames of %d x %d, forward + three gradients: HIP %.3f .. %.3f ms, torch autograd %.3f .. %.3f ms; "
              "kernels %s; largest differences / largest value: dx %.2e, dw %.2e, db %.2e"
              % (k, k, Ci, Co, B, H, W, *span(med["hip"]), *span(med["torch"]), kern or "not recorded by the profiler", diff["dx"], diff["dw"],
                 diff["db"]))
        print(json.dumps(rec), flush=True)
        del x, g, ours, ref


if __name__ == "__main__":
    main(sys.argv[1:])
