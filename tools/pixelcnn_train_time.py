"""Measurement: one training pass of the PixelCNN -- likelihood.ar_loss forward plus backward to every parameter -- for PixelSynth's
configuration on 32 x 32 grids at 16 and 64 frames (the reference's batch size), on its two routes.

    python tools/pixelcnn_train_time.py [--frames 16,64] [--grid 32] [--rounds 5] [--calls 5]

The "hip" route (csrc/pixelcnn_train.hip: PONO + skip + activation, the gate, the loss's backward; lmconv/train_ops.py) and the
"torch" route (the layers as plain torch, F.cross_entropy) alternate call by call on the same weights, codes and masks
(_measure.alternate): after 3 warm-up calls of each, a round is CALLS calls per route and gives one median per route; the range of the
rounds' medians is reported.  Then each route once more under torch's profiler, in a run of its own (_measure.device_events): the
device time of a call by class -- the masked convolutions (csrc/lmconv*.hip, both ways), the new kernels, the forward of the
loss (csrc/code_nll.hip), the nin products (what the BLAS launches, by its names), everything else --, the number of kernel launches
of a call, and, in a further run, torch.cuda.max_memory_allocated of a call.  The masked convolutions and the nin products are the
same code on both routes.  One JSON line per number of frames."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd import _lib, synthetic as syn  # noqa: E402
from pixelsynth_amd.likelihood import ar_loss  # noqa: E402
from pixelsynth_amd.lmconv import train_ops  # noqa: E402
from pixelsynth_amd.lmconv.layers import PONO  # noqa: E402
from pixelsynth_amd.lmconv.model import OurPixelCNN  # noqa: E402
from _measure import alternate, device_events, span  # noqa: E402

CLASSES = {
    "masked_convolutions": ("k_nchw_to_cl", "k_pack_conv", "k_gemm", "k_reduce_nchw", "k_to_cl", "k_grad_weight", "k_grad_bias", "k_adjoint_mask"),
    "new_kernels": ("k_norm_act_", "k_gate_", "k_nll_bwd_"),
    "loss_forward": ("k_code_nll_", "k_nll_frames"),
    "nin_products": ("Cijk", "gemm", "Gemm", "GEMM", "rocblas", "hipblas"),
}


def classify(name):
    return next((k for k, pats in CLASSES.items() if any(p in name for p in pats)), "rest")


def by_class(fn, calls):
    """-> (device ms of a call by class, kernel launches of a call by class, the six largest names of the rest) under torch's profiler"""
    ms, n, rest = dict.fromkeys(list(CLASSES) + ["rest"], 0.0), dict.fromkeys(list(CLASSES) + ["rest"], 0), {}
    for name, t in device_events(fn, calls):
        k = classify(name)
        ms[k] += t
        n[k] += 1
        if k == "rest":
            rest[name[:60]] = rest.get(name[:60], 0.0) + t
    top = sorted(rest.items(), key=lambda kv: -kv[1])[:6]
    return ({k: round(v / calls, 3) for k, v in ms.items()}, {k: round(v / calls, 1) for k, v in n.items()},
            [(name, round(v / calls, 3)) for name, v in top])


def peak_bytes(fn):
    fn()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated(), base


def masks_for(frames, grid, seed=0):
    """Random generation orders and their three masks, (F,9,L) each (ps_kernel_masks_f32: host code), and the region: the second half
    of each order is sampled"""
    L = grid * grid
    rs = np.random.RandomState(seed)
    masks = [np.empty((frames, 9, L), np.float32) for _ in range(3)]
    region = np.zeros((frames, L), np.uint8)
    for f in range(frames):
        order = np.ascontiguousarray(np.stack(np.unravel_index(rs.permutation(L), (grid, grid)), 1).astype(np.int32))
        for m, (dil, type_b) in zip(masks, ((1, 0), (1, 1), (2, 1))):
            one = np.empty((9, L), np.float32)
            _lib.call("ps_kernel_masks_f32", order, L, grid, grid, 3, dil, type_b, one)
            m[f] = one
        region[f, (order[:, 0] * grid + order[:, 1])[L // 2:]] = 1
    return [torch.from_numpy(m) for m in masks], torch.from_numpy(region)


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", default="16,64")
    ap.add_argument("--grid", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args(argv)
    device = torch.device("cuda", 0)
    net = OurPixelCNN(nr_resnet=2, nr_filters=80, input_channels=512, nr_logistic_mix=10, kernel_size=(3, 3), max_dilation=2, weight_norm=False,
                      feature_norm_op=lambda n: PONO(), dropout_prob=0, conv_bias=True, conv_mask_weight=False).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in syn.pixelcnn_state_dict(0).items()}, strict=True)
    net = net.to(device)
    params = list(net.parameters())
    for frames in (int(v) for v in args.frames.split(",")):
        masks, region = masks_for(frames, args.grid)
        masks, region = [m.to(device) for m in masks], region.to(device)
        codes = torch.from_numpy(np.random.RandomState(1).randint(0, 512, (frames, args.grid, args.grid))).to(device)

        def call(route):
            with train_ops.pixelcnn_train(route):
                loss = ar_loss(net, codes, masks, region=region)
            return loss, torch.autograd.grad(loss, params)

        med = alternate({"hip": lambda: call("hip"), "torch": lambda: call("torch")}, args.rounds, args.calls)
        (lh, gh), (lt, gt) = call("hip"), call("torch")
        diff = max(float((p - q).abs().max() / q.abs().max().clamp_min(1e-30)) for p, q in zip(gh, gt))
        lh, lt = lh.item(), lt.item()
        del gh, gt
        rec = dict(what="pixelcnn_train", frames=frames, grid=args.grid, rounds=args.rounds, calls=args.calls,
                   hip_ms_median_range=span(med["hip"]), torch_ms_median_range=span(med["torch"]), loss_hip=lh, loss_torch=lt,
                   max_grad_diff_over_max=diff, lanes_per_location=train_ops.lanes_per_location(frames * args.grid * args.grid))
        for route in ("hip", "torch"):
            ms, launches, top = by_class(lambda: call(route), args.calls)
            peak, base = peak_bytes(lambda: call(route))
            rec[route] = dict(device_ms_per_call=ms, device_ms_total=round(sum(ms.values()), 3), launches_per_call=launches,
                              launches_total=round(sum(launches.values()), 1), rest_top=top, max_memory_allocated_MiB=round(peak / 2 ** 20, 1),
                              allocated_before_MiB=round(base / 2 ** 20, 1))
        print("%d frames of %d x %d: medians of %d rounds of %d calls (forward + backward): hip %.3f .. %.3f ms, torch %.3f .. %.3f ms; losses "
              "%.6f / %.6f, largest gradient difference / largest value %.2e" % (frames, args.grid, args.grid, args.rounds, args.calls,
                                                                                *span(med["hip"]), *span(med["torch"]), lh, lt, diff))
        for route in ("hip", "torch"):
            r = rec[route]
            print("  %-5s device ms by class %s = %.3f; launches %s = %.0f; peak %.1f MiB (%.1f before the call)"
                  % (route, r["device_ms_per_call"], r["device_ms_total"], r["launches_per_call"], r["launches_total"],
                     r["max_memory_allocated_MiB"], r["allocated_before_MiB"]))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
