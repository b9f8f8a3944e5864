"""Measurement: likelihood.code_nll (csrc/code_nll.hip) on the logits of 128 frames of the 32 x 32 code grid, in both layouts, against the
torch formula on the same tensors -- log_softmax and gather for the nll, softmax * log_softmax for the entropy, argmax for the hit, the
sums per group with a mask -- and one score_codes call next to the engine's forward alone.

    python tools/nll_time.py [--frames 128] [--rounds 5] [--calls 20]

The logits are made once, outside the timed part (normal, magnitude 3).  The two routes alternate call by call (_measure.alternate):
after 3 warm-up calls of each, a round is CALLS calls per route and gives one median per route; the range of the rounds' medians is
reported.  The results of the two routes are compared, and the bytes the kernel
has to move over 8 TB/s are given as its lower bound.  One JSON line per layout and one for score_codes at the end."""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd import synthetic as syn  # noqa: E402
from pixelsynth_amd.likelihood import code_nll, score_codes  # noqa: E402
from pixelsynth_amd.lmconv.model import OurPixelCNN  # noqa: E402
from pixelsynth_amd.lmconv.layers import PONO  # noqa: E402
from _measure import alternate, span  # noqa: E402

HBM = 8.0e12
L = 1024


def torch_route(logits, targets, region, T, layout):
    """The same four outputs and the frame table from torch's own kernels -> (nll, entropy, hit, frames)"""
    dim = 1 if layout == "chw" else 2
    logp = torch.log_softmax(logits / T, dim)
    nll = -logp.gather(dim, targets.long().unsqueeze(dim)).squeeze(dim)
    entropy = -(torch.softmax(logits / T, dim) * logp).sum(dim)
    hit = (logits.argmax(dim) == targets).to(torch.uint8)
    g = region.bool()
    cols = torch.stack([torch.ones_like(nll, dtype=torch.float64), nll.double(), entropy.double(), hit.double()], -1)   # (F,L,4)
    frames = torch.stack([(cols * (~g)[..., None]).sum(1), (cols * g[..., None]).sum(1)], 1)
    return nll, entropy, hit, frames


def make_net(device):
    net = OurPixelCNN(nr_resnet=2, nr_filters=80, input_channels=512, nr_logistic_mix=10, kernel_size=(3, 3), max_dilation=2,
                      weight_norm=False, feature_norm_op=lambda c: PONO(), dropout_prob=0, conv_bias=True, conv_mask_weight=False,
                      rematerialize=False, binarize=False).eval()
    net.load_state_dict({k: torch.from_numpy(v) for k, v in syn.pixelcnn_state_dict(0).items()}, strict=True)
    return net.to(device)


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--frames", type=int, default=128)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--calls", type=int, default=20)
    args = ap.parse_args(argv)
    device = torch.device("cuda", 0)
    F_, T = args.frames, 0.7
    gen = torch.Generator(device="cpu").manual_seed(0)
    lc = (3.0 * torch.randn(F_, L, 512, generator=gen)).to(device)
    targets = torch.randint(0, 512, (F_, L), generator=gen, dtype=torch.int32).to(device)
    region = (torch.rand(F_, L, generator=gen) < 0.5).to(torch.uint8).to(device)
    with torch.no_grad():
        for layout, logits in (("chw", lc.permute(0, 2, 1).contiguous()), ("lc", lc)):
            med = alternate({"kernel": lambda: code_nll(logits, targets, region, T, layout),
                             "torch": lambda: torch_route(logits, targets, region, T, layout)}, args.rounds, args.calls)
            ours, ref = code_nll(logits, targets, region, T, layout), torch_route(logits, targets, region, T, layout)
            diff = dict(nll=float((ours.nll - ref[0]).abs().max()), entropy=float((ours.entropy - ref[1]).abs().max()),
                        hit=int((ours.hit != ref[2]).sum()), frames_rel=float(((ours.frames - ref[3]).abs() / ref[3].abs().clamp(min=1)).max()))
            moved = logits.numel() * 4 + F_ * L * (4 + 1 + 4 + 4 + 1) + F_ * L * (4 + 4 + 1 + 1)     # logits, targets, region, the three outputs, read again
            rec = dict(what="code_nll", layout=layout, frames=F_, L=L, temperature=T, rounds=args.rounds, calls=args.calls,
                       kernel_ms_median_range=span(med["kernel"]), torch_ms_median_range=span(med["torch"]),
                       bytes_bound_ms=round(moved / HBM * 1e3, 4), max_abs_diff=diff)
            print("code_nll %s, %d frames: medians of %d rounds of %d calls: kernel %.4f .. %.4f ms, torch formula %.4f .. %.4f ms; bytes / "
                  "8 TB/s = %.4f ms; largest difference nll %.3g, entropy %.3g, %d hits differ"
                  % (layout, F_, args.rounds, args.calls, *rec["kernel_ms_median_range"], *rec["torch_ms_median_range"], rec["bytes_bound_ms"],
                     diff["nll"], diff["entropy"], diff["hit"]))
            print(json.dumps(rec), flush=True)
        # one score_codes call next to its forward alone (the masks of the raster order: every location open to its predecessors)
        from pixelsynth_amd import _lib
        net = make_net(device)
        eng = net.engine(32, 32, F_)
        order = torch.arange(L, dtype=torch.int32, device=device).repeat(F_, 1).contiguous()
        masks = [torch.empty(F_, 9, L, dtype=torch.float32, device=device) for _ in range(3)]
        _lib.call("ps_order_masks_f32", order, F_, 32, 32, *masks, _lib.status_word(device))
        _lib.read_status("ps_order_masks_f32", device)
        codes = targets.view(F_, 32, 32)
        med = alternate({"forward": lambda: eng.forward(codes, *masks), "score_codes": lambda: score_codes(eng, codes, masks, region, T)},
                        args.rounds, max(args.calls // 4, 3))
        rec = dict(what="score_codes", frames=F_, rounds=args.rounds, calls=max(args.calls // 4, 3),
                   forward_ms_median_range=span(med["forward"]), score_codes_ms_median_range=span(med["score_codes"]))
        print("score_codes, %d frames: forward alone %.3f .. %.3f ms, score_codes %.3f .. %.3f ms"
              % (F_, *rec["forward_ms_median_range"], *rec["score_codes_ms_median_range"]))
        print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
