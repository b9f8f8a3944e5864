"""Measurement: the training-mode batch norm + ReLU of the refinement decoder (csrc/norm_train.hip through
networks/norm_train.py:batch_norm_train) at the decoder's own activation shapes -- 64 x 256^2, 128 x 256^2, 128 x 128^2, 256 x 128^2,
256 x 64^2 -- for B = 16 frames, against torch autograd of the same formula (m2 - m^2 statistics, x * scale - shift, ReLU) on the same
channels-last tensors.

    python tools/norm_train_time.py [--frames 16] [--rounds 5] [--calls 5] [--shapes 0,1,2,3,4]

A call is forward plus backward: y and the update of the stored statistics, then the gradients in x, gain and bias for one grad_output.
The two routes alternate call by call (_measure.alternate): after 3 warm-up calls of each, a round is CALLS calls per route and gives one
median per route; the range of the rounds' medians is reported.  The HIP route's kernels are the medians of their device times under
torch's profiler in a run of their own (_measure.device_events, kernel_medians), each with the bytes it has to move over
that time next to the 6.3 TB/s a float4 copy reaches on this GPU (MI355X_MICROARCH.md).  The two routes' gradients are compared on a
grad_output that is zero where the value in front of the ReLU is within 1e-4 of 0.  One JSON line per shape."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd import _lib  # noqa: E402
from pixelsynth_amd.networks import architectures as A, norm_train as NT  # noqa: E402
from _measure import alternate, device_events, kernel_medians, span  # noqa: E402

COPY_TBS = 6.3
SHAPES = ((64, 256), (128, 256), (128, 128), (256, 128), (256, 64))      # (C, H = W)
# kernel -> passes over the activation it reads or writes (the partial slabs and per-channel tables are a thousandth of that); in the
# order kernel_medians needs: k_stats_finish before k_stats
KERNELS = {"k_stats_finish": 0, "k_stats": 1, "k_apply": 2, "k_bwd_sums": 2, "k_bwd_frames": 0, "k_bwd_channels": 0, "k_bwd_dx": 3}


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
    for C, H in (SHAPES[int(i)] for i in args.shapes.split(",")):
        W = H
        x = (0.3 + 1.5 * torch.randn(B, C, H, W, generator=gen)).to(device).contiguous(memory_format=cl).requires_grad_()
        gain = (1 + 0.3 * torch.randn(B, C, generator=gen)).to(device).requires_grad_()
        bias = (0.3 * torch.randn(B, C, generator=gen)).to(device).requires_grad_()
        g = torch.randn(B, C, H, W, generator=gen).to(device).contiguous(memory_format=cl)
        layers = {"hip": A.bn(C).to(device).train(), "torch": A.bn(C).to(device).train()}

        def step(route, grad_y=g):
            with NT.decoder_norm_train(route):
                y = NT.batch_norm_train(x, gain, bias, layers[route], True)
            return torch.autograd.grad(y, (x, gain, bias), grad_y)

        def forward(route):
            with NT.decoder_norm_train(route), torch.no_grad():
                return NT.batch_norm_train(x, gain, bias, layers[route], True)
        routes = {"hip": lambda: step("hip"), "torch": lambda: step("torch"),
                  "hip_forward": lambda: forward("hip"), "torch_forward": lambda: forward("torch")}
        med = alternate(routes, args.rounds, args.calls)
        # the routes' gradients side by side, without the handful of the 10^7 .. 10^8 elements whose value in front of the ReLU is within
        # rounding of 0: there the two fp32 routes may set the mask differently, which is one whole term of a sum, not a rounding error
        with torch.no_grad(), NT.decoder_norm_train("torch"):
            near0 = NT.batch_norm_train(x, gain, bias, A.bn(C).to(device).train(), False).abs() < 1e-4
        gc = torch.where(near0, torch.zeros_like(g), g)
        masked = float(near0.float().mean())
        del near0
        ours, ref = step("hip", gc), step("torch", gc)
        diff = {k: float((p - q).abs().max() / q.abs().max()) for k, p, q in zip(("dx", "dgain", "dbias"), ours, ref)}
        kern = kernel_medians(device_events(routes["hip"], args.calls), KERNELS)
        act = 4.0 * B * C * H * W                                       # bytes of one pass over the activation
        rates = {k: round(KERNELS[k] * act / (t * 1e-3) / 1e12, 3) for k, t in kern.items() if KERNELS[k]}
        rec = dict(what="norm_relu_train", C=C, frames=B, H=H, W=W, rounds=args.rounds, calls=args.calls,
                   parts=_lib.call("ps_norm_train_parts", B, H * W, C), activation_bytes=act, kernel_ms_median=kern,
                   kernel_tb_per_s=rates, copy_tb_per_s=COPY_TBS, max_diff_over_max=diff, near_zero_fraction=masked,
                   **{f"{k}_ms_median_range": span(v) for k, v in med.items()})
        print("norm + ReLU, training mode, %d channels, %d frames of %d x %d: medians of %d rounds of %d calls: forward + backward HIP "
              "%.3f .. %.3f ms, torch autograd %.3f .. %.3f ms; forward alone HIP %.3f .. %.3f ms, torch %.3f .. %.3f ms; kernels %s; "
              "their bytes / time %s TB/s (a float4 copy: %.1f); largest differences / largest value (grad_output zeroed where |v| < 1e-4, %.1e of the elements): dx %.2e, dgain %.2e, dbias %.2e"
              % (C, B, H, W, args.rounds, args.calls, *span(med["hip"]), *span(med["torch"]), *span(med["hip_forward"]),
                 *span(med["torch_forward"]), kern or "not recorded by the profiler", rates or "-", COPY_TBS, masked, diff["dx"], diff["dgain"],
                 diff["dbias"]))
        print(json.dumps(rec), flush=True)
        del x, g, gc


if __name__ == "__main__":
    main(sys.argv[1:])
