"""Measurement: the depth regressor Unet in training, forward plus backward to every parameter, under unet_train("hip") against
unet_train("torch") (networks/unet_train.py, csrc/unet_train.hip, conv_routes._unet_train_conv).

    python tools/unet_train_time.py [--filters 32] [--batch 4 16] [--rounds 5] [--calls 5] [--layers]

Workload: Unet(32) in train(), B = 4 and 16 images of 256 x 256.  A call is one forward and the backward pass of a gradient of ones to
every parameter.  The two routes alternate call by call on the same network between device events (_measure.alternate): after 3 warm-up
calls of each, a round is CALLS calls per route and gives one median per route; the range of the ROUNDS medians is reported.  Both run
under spectral_train("hip"), so that the routes differ in the Unet's switch alone.  Then each route once more under torch's profiler,
in a run of its own (_measure.device_events): launches per call and device time per call by class -- the kernels of csrc/unet_train.hip,
the 3 x 3 products of this project (split-fp16, thin, their weight gradients and preparation), the library's convolutions, everything
else.  One JSON line per batch size.

--layers: dconv4 .. dconv8 alone, each as the route takes it (f16x3.conv3x3_train, thin_train.conv_thin_out_train; dconv7, which the
route leaves on torch, as its candidate: conv3x3_train on the weight and bias zero-padded to 64 output channels, the result narrowed to
32) against F.conv2d, forward + backward to the input, the weight and the bias, on an input of the layer's shape.  One JSON line per
layer and batch size."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd.networks import architectures as arch, f16x3, thin_train  # noqa: E402
from pixelsynth_amd.networks.spectral_train import spectral_train  # noqa: E402
from pixelsynth_amd.networks.unet_train import unet_train  # noqa: E402
from _measure import alternate, device_events, span  # noqa: E402

# csrc/unet_train.hip (k_stats_finish before k_stats: the first name found owns the event)
OURS = ("k_stats_finish", "k_stats", "k_apply", "k_bwd_sums", "k_bwd_finish", "k_bwd_dx", "k_up2_fwd", "k_up2_bwd")
PRODUCTS = ("k_conv3x3_f16x3", "k_pack", "k_prep_partial", "k_prep_finish", "k_scale", "k_grad_weight_parts", "k_grad_weight_sum", "k_thin_")
LIBRARY = ("conv", "Conv", "gemm", "Gemm", "GEMM", "Cijk", "igemm", "Igemm", "miopen", "MIOpen", "naive_", "gridwise", "col2im", "im2col",
           "Im2Col", "Col2Im", "wrw", "bwd_data", "xdlops", "SubTensorOp", "batched_transpose", "transpose_")
CLASSES = ("new kernels", "3 x 3 products", "library convolutions", "everything else")


def class_of(kernel):
    if any(k + "(" in kernel or kernel.endswith(k) for k in OURS):
        return "new kernels"
    if any(k in kernel for k in PRODUCTS):
        return "3 x 3 products"
    return "library convolutions" if any(k in kernel for k in LIBRARY) else "everything else"


def profile(fn, calls):
    events = device_events(fn, calls)
    totals = {c: 0.0 for c in CLASSES}
    for name, ms in events:
        totals[class_of(name)] += ms
    return dict(launches_per_call=len(events) // calls, device_ms_per_call={c: round(v / calls, 4) for c, v in totals.items()},
                device_ms_total=round(sum(totals.values()) / calls, 4))


def network(args, device):
    opt = argparse.Namespace(norm_G="sync:spectral_batch")
    torch.manual_seed(0)
    net = arch.Unet(num_filters=args.filters, channels_in=3, channels_out=3, opt=opt).to(device).train()
    params = list(net.parameters())
    for B in args.batch:
        x = torch.randn(B, 3, 256, 256, device=device)

        def call(route):
            with spectral_train("hip"), unet_train(route):
                y = net(x)
                return torch.autograd.grad(y, params, torch.ones_like(y))
        med = alternate({r: (lambda r=r: call(r)) for r in ("hip", "torch")}, args.rounds, args.calls)
        prof = {r: profile(lambda: call(r), args.calls) for r in ("hip", "torch")}
        rec = dict(what="unet_train", filters=args.filters, batch=B, rounds=args.rounds, calls=args.calls,
                   hip_ms_median_range=span(med["hip"]), torch_ms_median_range=span(med["torch"]), profile=prof)
        print("Unet(%d), %d images: medians of %d rounds of %d calls (forward + backward): hip %.3f .. %.3f ms, torch %.3f .. %.3f ms; launches "
              "per call hip %d / torch %d" % (args.filters, B, args.rounds, args.calls, *span(med["hip"]), *span(med["torch"]),
                                              prof["hip"]["launches_per_call"], prof["torch"]["launches_per_call"]))
        for c in CLASSES:
            print("  %-22s hip %8.3f ms   torch %8.3f ms" % (c, prof["hip"]["device_ms_per_call"][c], prof["torch"]["device_ms_per_call"][c]))
        print(json.dumps(rec), flush=True)


def padded(x, weight, bias):
    """dconv7's candidate: the weight and bias zero-padded to 64 output channels through conv3x3_train, the result narrowed"""
    Co = weight.size(0)
    w = torch.cat((weight, weight.new_zeros(64 - Co, *weight.shape[1:])))
    b = torch.cat((bias, bias.new_zeros(64 - Co)))
    return f16x3.conv3x3_train(x, w, b)[:, :Co]


def layers(args, device):
    f = args.filters
    # name: (Ci, Co, side, the route's form)
    table = {"dconv4": (16 * f, 8 * f, 16, f16x3.conv3x3_train), "dconv5": (16 * f, 4 * f, 32, f16x3.conv3x3_train),
             "dconv6": (8 * f, 2 * f, 64, f16x3.conv3x3_train), "dconv7": (4 * f, f, 128, padded),
             "dconv8": (2 * f, 3, 256, thin_train.conv_thin_out_train)}
    for B in args.batch:
        for name, (Ci, Co, side, form) in table.items():
            torch.manual_seed(1)
            x = torch.randn(B, Ci, side, side, device=device).contiguous(memory_format=torch.channels_last).requires_grad_()
            weight = (torch.randn(Co, Ci, 3, 3, device=device) / (3 * Ci ** 0.5)).contiguous(memory_format=torch.channels_last).requires_grad_()
            bias = torch.zeros(Co, device=device, requires_grad=True)

            def call(fn):
                y = fn(x, weight, bias)
                return torch.autograd.grad(y, (x, weight, bias), torch.ones_like(y))
            routes = {"hip": lambda: call(form), "torch": lambda: call(lambda x, w, b: F.conv2d(x, w, b, 1, 1))}
            med = alternate(routes, args.rounds, args.calls)
            rec = dict(what="unet_train_layer", layer=name, batch=B, Ci=Ci, Co=Co, side=side, form=form.__name__, rounds=args.rounds,
                       calls=args.calls, hip_ms_median_range=span(med["hip"]), torch_ms_median_range=span(med["torch"]))
            print("%s, %d images (%d -> %d at %d x %d, %s): hip %.3f .. %.3f ms, torch %.3f .. %.3f ms"
                  % (name, B, Ci, Co, side, side, form.__name__, *span(med["hip"]), *span(med["torch"])))
            print(json.dumps(rec), flush=True)


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--filters", type=int, default=32)
    ap.add_argument("--batch", type=int, nargs="+", default=[4, 16])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--layers", action="store_true")
    args = ap.parse_args(argv)
    device = torch.device("cuda", 0)
    (layers if args.layers else network)(args, device)


if __name__ == "__main__":
    main(sys.argv[1:])
