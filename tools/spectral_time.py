"""Measurement: the spectral normalisation of a network's layers in training, forward plus backward, at the weights of the full
configuration -- the refinement decoder (ngf = 64: 22 convolutions and 32 noise linears), the Unet (32 filters: 16 convolutions) and the
multiscale discriminator (ndf = 64: 6 _SNConvs) -- without the networks' own work: only the weights are touched.

    python tools/spectral_time.py [--ngf 64] [--unet 32] [--ndf 64] [--rounds 5] [--calls 5]

A call is one normalisation of every layer of a network in train() and the backward pass of a gradient of ones to every weight_orig.
The "hip" route (networks/spectral_train.normalise: one batched pass, csrc/spectral_train.hip) and the "torch" route (the legacy
torch.nn.utils.spectral_norm hook per layer; for the discriminator the same arithmetic in _SNConv.weight()) alternate call by call on the
same modules between device events (_measure.alternate): after 3 warm-up calls of each, a round is CALLS calls per route and gives one
median per route; the range of the rounds' medians is reported.  Then each route once more under torch's profiler, in a run of its own
(_measure.device_events): launches and device time per call, for "hip" by kernel.  Every call runs one power iteration on the stored
vectors, as a training step does.  One JSON line per network."""
import argparse
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd.networks import architectures as arch, conv_routes, discriminators as D, routing, spectral_train as ST  # noqa: E402
from _measure import alternate, device_events, span  # noqa: E402

OURS = ("k_sn_wtu", "k_sn_wv", "k_sn_v", "k_sn_u", "k_sn_div", "k_sn_dot", "k_sn_dw")


def networks(args):
    opt = argparse.Namespace(norm_G="sync:spectral_batch", refine_model_type="resnet_256W8UpDown3", ngf=args.ngf, isTrain=True,
                             norm_D="spectralinstance", ndf=args.ndf, output_nc=3, no_ganFeat_loss=False)
    torch.manual_seed(0)
    return {"decoder": arch.ResNetDecoder(opt, channels_in=4), "unet": arch.Unet(num_filters=args.unet, channels_in=3, channels_out=1, opt=opt),
            "discriminator": D.define_D(opt)}


def weight_of(mod):
    """The module's normalised weight as its forward asks for it: a pending one, else the hook's (or _SNConv's own arithmetic)"""
    if type(mod) is D._SNConv:
        return mod.weight()
    return conv_routes._normalised_weight(mod, conv_routes._sn_hooks(mod, type(mod)), None)


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--ngf", type=int, default=64)
    ap.add_argument("--unet", type=int, default=32)
    ap.add_argument("--ndf", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args(argv)
    device = torch.device("cuda", 0)
    for name, net in networks(args).items():
        net = net.to(device).to(memory_format=torch.channels_last).train()       # (the weights' storage on the GPU: architectures._nhwc)
        mods = [m for m in ST.sn_modules(net) if hasattr(m, "weight_orig")]
        ones = [torch.ones_like(m.weight_orig) for m in mods]

        def call(route):
            if route == "hip":
                assert len(ST.normalise(mods)) == len(mods)
            ws = [weight_of(m) for m in mods]
            assert not any(routing.has_pending(m) for m in mods)
            return torch.autograd.grad(ws, [m.weight_orig for m in mods], ones)

        med = alternate({"hip": lambda: call("hip"), "torch": lambda: call("torch")}, args.rounds, args.calls)
        prof = {}
        for route in ("hip", "torch"):
            events = device_events(lambda: call(route), args.calls)
            prof[route] = dict(launches_per_call=len(events) // args.calls, device_ms_per_call=round(sum(ms for _, ms in events) / args.calls, 4))
            if route == "hip":
                by = {}
                for ev, ms in events:
                    k = next((k for k in OURS if k + "(" in ev or ev.endswith(k)), None) or "other"
                    by.setdefault(k, []).append(ms)
                prof[route]["kernel_ms_median"] = {k: round(float(np.median(v)), 4) for k, v in by.items()}
        values = sum(m.weight_orig.numel() for m in mods)
        rec = dict(what="spectral_train", network=name, layers=len(mods), values=values, rounds=args.rounds, calls=args.calls,
                   hip_ms_median_range=span(med["hip"]), torch_ms_median_range=span(med["torch"]), profile=prof)
        print("%s: %d layers, %.1f M values: medians of %d rounds of %d calls (forward + backward): hip %.3f .. %.3f ms, torch %.3f .. %.3f ms; "
              "launches per call hip %d / torch %d, device ms per call hip %.3f / torch %.3f; hip kernels %s"
              % (name, len(mods), values / 1e6, args.rounds, args.calls, *span(med["hip"]), *span(med["torch"]),
                 prof["hip"]["launches_per_call"], prof["torch"]["launches_per_call"], prof["hip"]["device_ms_per_call"],
                 prof["torch"]["device_ms_per_call"], prof["hip"].get("kernel_ms_median")))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
