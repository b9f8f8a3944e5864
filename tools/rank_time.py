"""Measurement: scoring and ranking the best-of-N candidates of a view per route -- rank_on="host" (one candidate at a time through the
host: the discriminator next to the input image, the classifier's input by numpy and Pillow, the rank rule in numpy) against
rank_on="device" (ranking.score_candidates + ranking.select: one batch, nothing comes down but the winner's index, read here to end the
timing) -- on the scorer mirrors with synthetic weights.

    python tools/rank_time.py [N ...]        (default: 4 16 50)
    python tools/rank_time.py --views B [N ...]   per-view ranking of N x B candidates (ranking.score_candidates in chunks,
                                                  select_groups, take_groups: get_best_sample's rank_scope="view") against B calls of
                                                  the B = 1 device route above, one per view; each ends at a synchronised device

The N candidates (256 x 256, U(-1,1)) are made once, outside the timed part: decoding is the same on both routes and is not measured.
Per route: WARM invocations, then CALLS timed ones, each from a synchronised device to the winner's index on the host; the routes
alternate invocation by invocation, in one process.  Wall time per invocation as min / median / max, and the largest difference
between the two routes' scores.  One JSON line per N at the end."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pixelsynth_amd import ranking  # noqa: E402
from pixelsynth_amd import synthetic as syn  # noqa: E402
from pixelsynth_amd.losses import DiscriminatorLoss  # noqa: E402
from pixelsynth_amd.networks import resnet18  # noqa: E402
from pixelsynth_amd.z_buffermodel import ZbufferModelPts, rank_samples  # noqa: E402

WARM, CALLS = 1, 3


def scorers(device):
    torch.manual_seed(0)
    classifier = resnet18(num_classes=365).eval().to(device)
    opt = argparse.Namespace(discriminator_losses="pix2pixHD", gan_mode="hinge", norm_D="spectralinstance", ndf=64, output_nc=3,
                             no_ganFeat_loss=False, isTrain=False, lambda_feat=10.0)
    netD = DiscriminatorLoss(opt).eval()
    shapes = {k: tuple(v.shape) for k, v in netD.state_dict().items()}
    netD.load_state_dict({k: torch.from_numpy(v) for k, v in syn.fill_state_dict(shapes, 9).items()}, strict=True)
    return netD.to(device), classifier


def host_route(cands, real, netD, holder):
    """get_best_sample's host lines on decoded candidates -> (winner, disc, entr)"""
    disc, entr = [], []
    for img in cands:
        disc.append(float(netD.run_discriminator_one_step(img, real)["D_Fake"].mean().cpu()))
        entr.append(holder._entropy_score(img))
    return rank_samples(disc, entr), disc, entr


def device_route(cands, netD, classifier):
    """get_best_sample's device lines on decoded candidates -> (winner, disc, entr); the index is read to end the timing"""
    stack = torch.cat(cands)
    disc, entr = ranking.score_candidates(stack, netD, classifier)
    best = ranking.select(disc, entr)
    stack.index_select(0, best)
    return int(best), disc, entr


def per_view_route(stack, views, N, netD, classifier):
    """get_best_sample's rank_scope="view" lines on the decoded (N * views,3,S,S) candidate-major stack -> (winners (views,3,S,S), disc, entr)"""
    disc, entr = ranking.score_candidates(stack, netD, classifier, ranking.SCORE_CHUNK)
    return ranking.take_groups(stack, ranking.select_groups(disc, entr, views, N), N), disc, entr


def time_views(views, counts, device, netD, classifier):
    """--views: N x B candidates ranked per view in one go against B calls of the B = 1 device route; one JSON line per N"""
    for N in counts:
        stack = torch.cat([torch.from_numpy(syn.image(100 + i, views, 3, 256)) for i in range(N)]).to(device)   # candidate-major
        alone = [[stack[i * views + b:i * views + b + 1] for i in range(N)] for b in range(views)]
        wall, last = {"per_view": [], "one_by_one": []}, {}
        for rep in range(WARM + CALLS):
            for route in wall:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                if route == "per_view":
                    last[route] = per_view_route(stack, views, N, netD, classifier)
                else:
                    last[route] = [device_route(c, netD, classifier) for c in alone]
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                if rep >= WARM:
                    wall[route].append(1e3 * (t1 - t0))
        stat = lambda x: [round(float(f(x)), 3) for f in (np.min, np.median, np.max)]
        winners, disc, entr = last["per_view"]
        want = [r[0] for r in last["one_by_one"]]
        same = sum(bool(torch.equal(winners[b], stack[want[b] * views + b])) for b in range(views))
        diff = [max(float((last["per_view"][k].view(N, views)[:, b] - last["one_by_one"][b][k]).abs().max()) for b in range(views))
                for k in (1, 2)]
        rec = dict(N=N, views=views, calls=CALLS, chunk=ranking.SCORE_CHUNK, per_view_wall_ms=stat(wall["per_view"]),
                   one_by_one_wall_ms=stat(wall["one_by_one"]), max_abs_diff_disc=diff[0], max_abs_diff_entropy=diff[1],
                   same_winners=same, cpus=len(os.sched_getaffinity(0)))
        print("N=%d views=%d  scoring + ranking wall per invocation (min / median / max of %d): per view %.2f / %.2f / %.2f ms, %d calls of "
              "the B = 1 device route %.2f / %.2f / %.2f ms; largest difference of a score: D_Fake %.3g, entropy %.3g; %d of %d winners alike"
              % (N, views, CALLS, *rec["per_view_wall_ms"], views, *rec["one_by_one_wall_ms"], diff[0], diff[1], same, views))
        print(json.dumps(rec), flush=True)


def main(argv):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("counts", nargs="*", type=int, metavar="N", help="candidates per view (default: 4 16 50)")
    ap.add_argument("--views", type=int, metavar="B", help="rank N x B candidates per view against B calls of the B = 1 device route")
    args = ap.parse_args(argv)
    counts = args.counts or [4, 16, 50]
    device = torch.device("cuda", 0)
    netD, classifier = scorers(device)
    if args.views is not None:
        if args.views < 1:
            ap.error("--views must be >= 1")
        with torch.no_grad():
            time_views(args.views, counts, device, netD, classifier)
        return
    holder = type("H", (), {"classifier": classifier, "_entropy_score": ZbufferModelPts._entropy_score})()
    real = torch.from_numpy(syn.image(31, 1, 3, 256)).to(device)
    with torch.no_grad():
        for N in counts:
            cands = [torch.from_numpy(syn.image(100 + i, 1, 3, 256)).to(device) for i in range(N)]
            wall, last = {"host": [], "device": []}, {}
            for rep in range(WARM + CALLS):
                for route in wall:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    last[route] = host_route(cands, real, netD, holder) if route == "host" else device_route(cands, netD, classifier)
                    t1 = time.perf_counter()
                    if rep >= WARM:
                        wall[route].append(1e3 * (t1 - t0))
            stat = lambda x: [round(float(f(x)), 3) for f in (np.min, np.median, np.max)]
            diff = [float(np.abs(np.asarray(last["host"][k]) - last["device"][k].cpu().numpy()).max()) for k in (1, 2)]
            rec = dict(N=N, calls=CALLS, host_wall_ms=stat(wall["host"]), device_wall_ms=stat(wall["device"]),
                       host_ms_per_candidate=round(float(np.median(wall["host"])) / N, 3), max_abs_diff_disc=diff[0],
                       max_abs_diff_entropy=diff[1], same_winner=last["host"][0] == last["device"][0], cpus=len(os.sched_getaffinity(0)))
            print("N=%d  scoring + ranking wall per invocation (min / median / max of %d): host %.2f / %.2f / %.2f ms, device %.2f / %.2f / "
                  "%.2f ms; largest |host - device|: D_Fake %.3g, entropy %.3g"
                  % (N, CALLS, *rec["host_wall_ms"], *rec["device_wall_ms"], diff[0], diff[1]))
            print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main(sys.argv[1:])
