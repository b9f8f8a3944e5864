"""Measurement: one training pass of the multiscale discriminator (networks/discriminators.py and losses/gan_loss.py with opt.isTrain) at
the reference's training workload -- B = 16 pairs of 256 x 256, ndf = 64 -- in its two modes: (a) the generator's, hinge + feature
matching with the gradient to the fake image, (b) the discriminator's, hinge on fake and real with the gradients to its parameters.

    python tools/gan_train_time.py [--pairs 16] [--size 256] [--ndf 64] [--rounds 5] [--calls 5]

A call is forward plus backward of the mode's total.  The "hip" route (csrc/gan_train.hip: instance norm + LeakyReLU and the feature
matching) and the "torch" route (F.instance_norm + F.leaky_relu, F.l1_loss per map, autograd's backward) alternate call by call on the
same weights and images (_measure.alternate): after 3 warm-up calls of each, a round is CALLS calls per route and gives one median per
route; the range of the rounds' medians is reported.  Then the "hip" route once more under torch's profiler, in a run of its own
(_measure.device_events): the device time of the new kernels by name, of the convolutions (what MIOpen and the BLAS
launch, by their names) and of everything else, as shares of a call.  The convolutions are torch's on both routes.  The two routes'
gradients are compared twice: as they are, and with no gradient through the elements within NEAR of a kink -- of the LeakyReLU behind
a norm, of |f - r| in the feature matching -- where two fp32 evaluations may decide differently.  One JSON line per mode."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd import synthetic as syn  # noqa: E402
from pixelsynth_amd.losses import DiscriminatorLoss  # noqa: E402
from pixelsynth_amd.networks import gan_train as GT  # noqa: E402
from _measure import alternate, device_events, span  # noqa: E402

NEAR = 1e-4        # |v| below which a normalised value counts as next to the LeakyReLU's kink in the routes' comparison
OURS = ("k_norm_fwd_stream", "k_norm_bwd_stream", "k_norm_fwd", "k_norm_bwd", "k_feat_tiles", "k_feat_finish", "k_feat_bwd")
CONV_NAMES = ("conv", "Conv", "gemm", "Gemm", "GEMM", "Cijk", "igemm", "Igemm", "miopen", "MIOpen", "naive_", "gridwise", "col2im", "im2col",
              "Im2Col", "Col2Im", "wrw", "bwd_data", "xdlops", "SubTensorOp", "batched_transpose", "transpose_")


def shares(fn, calls):
    """{new kernel: median device ms per launch}, and the device ms of a call by class: ours, convolutions, the rest"""
    ours, total = {}, dict(ours=0.0, convolutions=0.0, rest=0.0)
    rest_names = {}
    for name, ms in device_events(fn, calls):
        mine = next((k for k in OURS if k in name), None)
        if mine:
            ours.setdefault(mine, []).append(ms)
            total["ours"] += ms
        elif any(s in name for s in CONV_NAMES):
            total["convolutions"] += ms
        else:
            total["rest"] += ms
            rest_names[name[:60]] = rest_names.get(name[:60], 0.0) + ms
    top = sorted(rest_names.items(), key=lambda kv: -kv[1])[:6]
    return ({k: [round(float(np.median(v)), 4), len(v) // calls] for k, v in ours.items()}, {k: round(v / calls, 3) for k, v in total.items()},
            [(n, round(v / calls, 3)) for n, v in top])


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--pairs", type=int, default=16)
    ap.add_argument("--size", type=int, default=256)
    ap.add_argument("--ndf", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=5)
    args = ap.parse_args(argv)
    device = torch.device("cuda", 0)
    opt = argparse.Namespace(discriminator_losses="pix2pixHD", gan_mode="hinge", norm_D="spectralinstance", ndf=args.ndf, output_nc=3,
                             no_ganFeat_loss=False, isTrain=True, lambda_feat=10.0, lr=1e-4)
    net = DiscriminatorLoss(opt).train()
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    net.load_state_dict({k: torch.from_numpy(v) for k, v in syn.fill_state_dict(shapes, 8).items()}, strict=True)
    net = net.to(device)
    fake = torch.from_numpy(syn.image(31, args.pairs, 3, args.size)).to(device).requires_grad_()
    real = torch.from_numpy(syn.image(32, args.pairs, 3, args.size)).to(device)
    params = list(net.parameters())

    def call(mode, route):
        with GT.discriminator_train(route):
            if mode == "generator":
                loss = net.run_generator_one_step(fake, real)["Total Loss"].mean()
                return loss, torch.autograd.grad(loss, [fake] + params)
            loss = net.run_discriminator_one_step(fake, real)["Total Loss"].mean()
            return loss, torch.autograd.grad(loss, params)

    for mode in ("generator", "discriminator"):
        med = alternate({"hip": lambda: call(mode, "hip"), "torch": lambda: call(mode, "torch")}, args.rounds, args.calls)
        # the routes' results side by side (every call runs one power iteration on the stored vectors; after the calls above they are at
        # their fixed point to rounding)
        (lh, gh), (lt, gt) = call(mode, "hip"), call(mode, "torch")
        lh, lt = lh.item(), lt.item()
        names = (["fake image"] if mode == "generator" else []) + [k for k, _ in net.named_parameters()]
        diffs = {k: float((p - q).abs().max() / q.abs().max().clamp_min(1e-30)) for k, p, q in zip(names, gh, gt)}
        worst = max(diffs, key=diffs.get)
        diff = diffs[worst]
        # ... and once more with no gradient through the normalised values within NEAR of the LeakyReLU's kink, nor through the feature
        # values within NEAR of their real partner, the kink of |f - r| (the same elements on both routes: the masks of the torch call):
        # what is left of the difference is rounding, what went is the branches and signs the two fp32 routes decide differently, each a
        # whole term of a gradient's sum
        masks, at, plain = [], [0], GT.instance_norm_lrelu_train
        fmasks, fplain = [], GT.feature_matching

        def feat_masked(maps, weight, opt=None, per_map=False):
            if not fmasks:
                for m in maps:
                    half = m.size(0) // 2
                    tie = (m[:half] - m[half:]).detach().abs() < NEAR
                    fmasks.append(torch.cat([tie, tie]))
            return fplain([torch.where(k, m.detach(), m) for k, m in zip(fmasks, maps)], weight, opt, per_map)

        def masked(x, eps=1e-5, slope=0.2, opt=None):
            y = plain(x, eps, slope, opt)
            if at[0] == len(masks):
                masks.append((y.detach() < NEAR) & (y.detach() > -slope * NEAR))
            at[0] += 1
            return torch.where(masks[at[0] - 1], y.detach(), y)
        GT.instance_norm_lrelu_train, GT.feature_matching = masked, feat_masked
        try:
            _, gt_m = call(mode, "torch")
            at[0] = 0
            _, gh_m = call(mode, "hip")
        finally:
            GT.instance_norm_lrelu_train, GT.feature_matching = plain, fplain
        diff_m = max(float((p - q).abs().max() / q.abs().max().clamp_min(1e-30)) for p, q in zip(gh_m, gt_m))
        near = sum(int(m.sum()) for m in masks) / sum(m.numel() for m in masks)
        ties = sum(int(m.sum()) for m in fmasks) / max(1, sum(m.numel() for m in fmasks))
        del masks, fmasks, gt_m, gh_m
        kern, total, rest = shares(lambda: call(mode, "hip"), args.calls)
        all_ms = sum(total.values())
        rec = dict(what="discriminator_train", mode=mode, pairs=args.pairs, size=args.size, ndf=args.ndf, rounds=args.rounds, calls=args.calls,
                   hip_ms_median_range=span(med["hip"]), torch_ms_median_range=span(med["torch"]), loss_hip=float(lh), loss_torch=float(lt),
                   max_grad_diff_over_max=diff, max_grad_diff_at=worst, grad_diff_over_max={k: float("%.3g" % v) for k, v in diffs.items()},
                   max_grad_diff_over_max_without_kinks=diff_m, near_kink_fraction=near, near_tie_fraction=ties,kernel_ms_median_and_launches=kern, device_ms_per_call=total,
                   share={k: round(v / all_ms, 3) for k, v in total.items()} if all_ms else {}, rest_top=rest)
        print("%s mode, %d pairs of %d x %d, ndf %d: medians of %d rounds of %d calls (forward + backward): hip %.3f .. %.3f ms, torch %.3f .. "
              "%.3f ms; losses %.6f / %.6f, largest gradient difference / largest value %.2e (%s), with no gradient through the %.1e of the normalised values and the %.1e of the feature "
              "differences within %g of their kink %.2e; device ms of a hip call: %s; new kernels %s"
              % (mode, args.pairs, args.size, args.size, args.ndf, args.rounds, args.calls, *span(med["hip"]), *span(med["torch"]), float(lh),
                 float(lt), diff, worst, near, ties, NEAR, diff_m, total, kern or "not recorded by the profiler"))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
