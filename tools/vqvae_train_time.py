"""Measurement: one training step of the VQ-VAE under vqvae_train("hip") against vqvae_train("torch") (vqvae2/conv_train.py,
csrc/vq_conv_train.hip, vqvae2/train.py).

    python tools/vqvae_train_time.py [--batch 16 64] [--rounds 5] [--calls 5]

Workload: VQVAETop() in train(), B = 16 and 64 images of 256 x 256, Adam.  A call is one vqvae2.train.train_step: forward, backward to
every parameter, the overflow check of the "hip" route, the optimiser's step and the two read-backs of the losses.  The two routes
alternate call by call on the same network in one process between device events (_measure.alternate): after 3 warm-up calls of each, a
round is CALLS calls per route and gives one median per route; the range of the ROUNDS medians is reported.  The "torch" route is the
parent route of this network: the yardstick lies in the same process.  Then each route once more under torch's profiler, in a run of
its own (_measure.device_events): launches per call and device time per call by class -- the kernels of csrc/vq_conv_train.hip, the
matrix products of this project (split-fp16 3 x 3 and its weight gradient, the fp32 1 x 1 and its weight gradient, the ends' forward
kernels), the quantiser's kernels, the library's convolutions, everything else -- and the peak of allocated device memory of a call.
One JSON line per batch size."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd.vqvae2 import VQVAETop, vqvae_train  # noqa: E402
from pixelsynth_amd.vqvae2.train import train_step  # noqa: E402
from _measure import alternate, device_events, span  # noqa: E402

OURS = ("k_relu_pack", "k_gate", "k_fold", "k_ends_grad_weight", "k_ends_sum_parts", "k_head_grad_input")      # csrc/vq_conv_train.hip
PRODUCTS = ("k_conv3x3_f16x3", "k_pack", "k_prep_partial", "k_prep_finish", "k_scale", "k_grad_weight_parts", "k_grad_weight_sum",
            "k_conv1x1", "k_vq_stem", "k_vq_head", "k_unscale")
QUANTISER = ("k_vq_", "k_nearest", "k_embed")
LIBRARY = ("conv", "Conv", "gemm", "Gemm", "GEMM", "Cijk", "igemm", "Igemm", "miopen", "MIOpen", "naive_", "gridwise", "col2im", "im2col",
           "Im2Col", "Col2Im", "wrw", "bwd_data", "xdlops", "SubTensorOp", "batched_transpose", "transpose_")
CLASSES = ("new kernels", "matrix products", "quantiser", "library convolutions", "everything else")


def class_of(kernel):
    if any(k in kernel for k in OURS):
        return "new kernels"
    if any(k in kernel for k in PRODUCTS):
        return "matrix products"
    if any(k in kernel for k in QUANTISER):
        return "quantiser"
    return "library convolutions" if any(k in kernel for k in LIBRARY) else "everything else"


def profile(fn, calls):
    events = device_events(fn, calls)
    totals = {c: 0.0 for c in CLASSES}
    for name, ms in events:
        totals[class_of(name)] += ms
    return dict(launches_per_call=len(events) // calls, device_ms_per_call={c: round(v / calls, 4) for c, v in totals.items()},
                device_ms_total=round(sum(totals.values()) / calls, 4))


def peak_mib(fn):
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return round(torch.cuda.max_memory_allocated() / 2 ** 20, 1)


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--batch", type=int, nargs="+", default=[16, 64])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args(argv)
    device = torch.device("cuda", 0)
    for B in args.batch:
        torch.manual_seed(0)
        model = VQVAETop().to(device).train()
        optimizer = torch.optim.Adam(model.parameters(), lr=3e-4)
        img = torch.rand(B, 3, 256, 256, device=device)

        def call(route):
            with vqvae_train(route):
                return train_step(model, optimizer, img)
        routes = {r: (lambda r=r: call(r)) for r in ("hip", "torch")}
        med = alternate(routes, args.rounds, args.calls)
        prof = {r: profile(routes[r], args.calls) for r in routes}
        peak = {r: peak_mib(routes[r]) for r in routes}
        rec = dict(what="vqvae_train_step", batch=B, rounds=args.rounds, calls=args.calls, hip_ms_median_range=span(med["hip"]),
                   torch_ms_median_range=span(med["torch"]), profile=prof, peak_mib=peak)
        print("VQVAETop, %d images: medians of %d rounds of %d train_steps: hip %.3f .. %.3f ms, torch %.3f .. %.3f ms; launches per call "
              "hip %d / torch %d; peak memory hip %.1f / torch %.1f MiB"
              % (B, args.rounds, args.calls, *span(med["hip"]), *span(med["torch"]), prof["hip"]["launches_per_call"],
                 prof["torch"]["launches_per_call"], peak["hip"], peak["torch"]))
        for c in CLASSES:
            print("  %-22s hip %8.3f ms   torch %8.3f ms" % (c, prof["hip"]["device_ms_per_call"][c], prof["torch"]["device_ms_per_call"][c]))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
