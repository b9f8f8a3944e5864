"""Measurement: one training forward and backward of the VQ-VAE's quantiser alone (csrc/vq_train.hip through Quantize.forward in train()
mode) at the reference's two levels for a batch of 64 images -- (N, D, K) = (65 536, 64, 512), the top level, and (262 144, 64, 512),
the bottom level -- against the torch formula of the reference's Quantize.forward (an (N, K) distance matrix, its arg-min, an (N, K)
one-hot, two dense products against it, the EMA update, the straight-through output) on the device.

    python tools/vq_train_time.py [--rounds 5] [--calls 10]

Both routes compute quantize, diff and the codes, update the three buffers, and take the gradient with respect to the input for the same
grad_quantize and grad_diff.  The routes alternate call by call (_measure.alternate): after 3 warm-up calls of each, a round is CALLS calls
per route and gives one median per route; the range of the rounds' medians is reported.  Beside the two whole routes: each with the codes GIVEN (what follows the arg-min), and ps_vq_nearest_f32 alone.  One JSON
line per shape."""
import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd.vqvae2.vqvae import Quantize  # noqa: E402
from _measure import alternate, span  # noqa: E402

SHAPES = ((65536, 64, 512), (262144, 64, 512))


def torch_quantize(q, z, codes=None):
    """The reference's training forward restated in torch on the buffers of q: the distance matrix and its arg-min (skipped where the
    codes are given), the float one-hot matrix, its column sums and its product with the latents, the EMA update, the straight-through
    output and the commitment term"""
    D, K, decay = q.dim, q.n_embed, q.decay
    flat = z.reshape(-1, D)
    book = q.embed
    if codes is None:
        dist = (flat * flat).sum(1, keepdim=True) - 2 * (flat @ book) + (book * book).sum(0, keepdim=True)
        codes = dist.argmin(1)
    onehot = F.one_hot(codes, K).to(flat.dtype)
    chosen = book.t()[codes].view(z.shape)
    q.cluster_size.mul_(decay).add_(onehot.sum(0), alpha=1 - decay)
    q.embed_avg.mul_(decay).add_(flat.t() @ onehot, alpha=1 - decay)
    total = q.cluster_size.sum()
    smoothed = (q.cluster_size + q.eps) / (total + K * q.eps) * total
    q.embed.copy_(q.embed_avg / smoothed)
    residual = (chosen - z).detach()
    return z + residual, (z - chosen.detach()).pow(2).mean(), codes


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=10)
    args = ap.parse_args(argv)
    device = torch.device("cuda", 0)
    gen = torch.Generator(device="cpu").manual_seed(0)
    for N, D, K in SHAPES:
        z = torch.randn(N, D, generator=gen).to(device).requires_grad_()
        gq = torch.randn(N, D, generator=gen).to(device)
        gd = torch.tensor(0.25, device=device)
        start = Quantize(D, K).to(device).train().state_dict()

        def module(given=None):
            q = Quantize(D, K).to(device).train()
            q.load_state_dict(start)
            if given is not None:                                   # (the arg-min skipped: the codes of the first call, kept)
                q.nearest = lambda flat, layout, hw=1: given
            return q

        def step(forward):
            quantize, diff, codes = forward()
            return (quantize.detach(), diff.detach(), codes) + torch.autograd.grad((quantize, diff), z, (gq, gd))

        # the two routes from the same state: what they disagree by
        q_hip, q_torch = module(), module()
        ours, theirs = step(lambda: q_hip(z)), step(lambda: torch_quantize(q_torch, z))
        codes = ours[2]
        same = codes == theirs[2]
        diffs = dict(codes_that_differ=int((~same).sum()),
                     quantize=float((ours[0] - theirs[0])[same].abs().max()), diff=float((ours[1] - theirs[1]).abs()),
                     grad_input=float((ours[3] - theirs[3])[same].abs().max()),
                     embed_relative=float(((q_hip.embed - q_torch.embed).abs() / q_torch.embed.abs().clamp_min(1e-30)).median()))
        q_given, q_torch_given = module(codes.to(torch.int32)), module()
        routes = {"hip": lambda: step(lambda: q_hip(z)),
                  "torch": lambda: step(lambda: torch_quantize(q_torch, z)),
                  "hip_given_codes": lambda: step(lambda: q_given(z)),
                  "torch_given_codes": lambda: step(lambda: torch_quantize(q_torch_given, z, codes)),
                  "nearest": lambda: q_hip.nearest(z.detach(), 0)}
        med = alternate(routes, args.rounds, args.calls)
        rec = dict(what="vq_train", N=N, D=D, K=K, rounds=args.rounds, calls=args.calls, stats_flop=2.0 * D * K * N, differences=diffs,
                   **{f"{k}_ms_median_range": span(v) for k, v in med.items()})
        print("quantiser training step, N = %d, D = %d, K = %d: medians of %d rounds of %d calls: HIP %.3f .. %.3f ms (codes given "
              "%.3f .. %.3f, ps_vq_nearest_f32 alone %.3f .. %.3f), the reference's torch formula %.3f .. %.3f ms (codes given "
              "%.3f .. %.3f); %d of the codes differ, largest differences elsewhere: quantize %.3g, diff %.3g, grad_input %.3g"
              % (N, D, K, args.rounds, args.calls, *span(med["hip"]), *span(med["hip_given_codes"]), *span(med["nearest"]),
                 *span(med["torch"]), *span(med["torch_given_codes"]), diffs["codes_that_differ"], diffs["quantize"], diffs["diff"],
                 diffs["grad_input"]))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
