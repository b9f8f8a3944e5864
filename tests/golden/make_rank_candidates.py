"""Makes tests/golden/rank_candidates.npz: four fixed candidates for the GPU test that runs both ranking routes of get_best_sample's
scorers on the real mirrors (tests/test_rank_device_gpu.py).

    python tests/golden/make_rank_candidates.py          (CPU, a few minutes; the mirrors run there)

The test wants the HOST route's scores of the four candidates at least 1e-2 apart in both lists, so that the routes' allowance of 1e-4
per score cannot touch the order.  With the weights the test uses -- the multiscale discriminator filled by
synthetic.fill_state_dict(shapes, 9) and the ResNet-18 as torch.manual_seed(0) initialises it -- no seeded noise, ramp, stripe or flat
picture in [-1,1] gets there: over such pictures the entropy stays within 2e-3 of ln 365 and D_Fake within 0.03 of 0.97.  So the
candidates are optimised instead: four (3,256,256) patterns are moved by Adam until each candidate's two scores sit on its targets.  The entropy's gradient goes through the resample as a matrix product with Pillow's weights
(ranking.pil_bilinear_tables) without its 8-bit rounding; every few steps the targets are corrected by what the true host score says.
A pattern is stored as int8 levels q in -7 .. 7 (fifteen levels: the file packs to half a byte per value), the candidate is the fp32
quotient q / 7 -- so the file fixes the candidates bit for bit -- and the script ends by checking the gaps on the true host scores of
what it stored.
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from pixelsynth_amd import ranking, synthetic as syn  # noqa: E402
from pixelsynth_amd.losses import DiscriminatorLoss  # noqa: E402
from pixelsynth_amd.networks import resnet18  # noqa: E402
from pixelsynth_amd.z_buffermodel import ZbufferModelPts  # noqa: E402

ENTROPY_TARGETS = (5.8990, 5.8880, 5.8770, 5.8660)      # 1.1e-2 apart
D_FAKE_TARGETS = (0.970, 0.955, 1.000, 0.985)           # 1.5e-2 apart, in another order than the entropies
LEVELS = 7
TOLERANCE = (2e-3, 1e-3)                                 # of D_Fake and of the entropy, see main


def scorers():
    """The weights of test_get_best_sample_runs_end_to_end_with_the_real_scorers, on the CPU"""
    torch.manual_seed(0)
    classifier = resnet18(num_classes=365).eval()
    opt = argparse.Namespace(discriminator_losses="pix2pixHD", gan_mode="hinge", norm_D="spectralinstance", ndf=64, output_nc=3,
                             no_ganFeat_loss=False, isTrain=False, lambda_feat=10.0)
    netD = DiscriminatorLoss(opt).eval()
    shapes = {k: tuple(v.shape) for k, v in netD.state_dict().items()}
    netD.load_state_dict({k: torch.from_numpy(v) for k, v in syn.fill_state_dict(shapes, 9).items()}, strict=True)
    for p in list(classifier.parameters()) + list(netD.parameters()):
        p.requires_grad_(False)
    return netD, classifier


def candidates(levels):
    """int8 (4,3,256,256) -> the candidates, fp32 in [-1,1]"""
    return torch.from_numpy(levels.astype(np.float32) / np.float32(LEVELS))


def host_scores(imgs, netD, classifier, real):
    """The host route's two scores of every candidate, as get_best_sample forms them"""
    holder = type("H", (), {"classifier": classifier, "_entropy_score": ZbufferModelPts._entropy_score})()
    with torch.no_grad():
        disc = [float(netD.run_discriminator_one_step(imgs[i:i + 1], real)["D_Fake"].mean()) for i in range(len(imgs))]
        entr = [holder._entropy_score(imgs[i:i + 1]) for i in range(len(imgs))]
    return np.array(disc), np.array(entr)


def smooth_scores(imgs, netD, classifier, weights):
    """The same two scores with a gradient: the resample as a matrix product with Pillow's weights, no rounding to bytes"""
    S = imgs.shape[-1]
    picture = imgs.reshape(-1, S, S, 3).permute(0, 3, 1, 2) * .5 + .5              # the reference's reshape, then planar for the product
    small = torch.einsum("ty,ncyx,ux->nctu", weights, picture, weights)
    mean, std = (torch.tensor(v).view(1, 3, 1, 1) for v in (ranking.MEAN, ranking.STD))
    p = torch.softmax(classifier((small - mean) / std), 1)
    entr = -(p * torch.log(p)).sum(1)
    maps = [scale[-1] for scale in netD.netD.netD(imgs)]
    disc = sum(-torch.clamp(-m - 1, max=0).flatten(1).mean(1) for m in maps) / len(maps)
    return disc, entr


def main(steps=400, out=os.path.join(HERE, "rank_candidates.npz")):
    netD, classifier = scorers()
    real = torch.from_numpy(syn.image(31, 1, 3, 256))
    bounds, coeffs = ranking.pil_bilinear_tables(256, 224)
    weights = torch.zeros(224, 256)
    for i, (lo, count) in enumerate(bounds):
        weights[i, lo:lo + count] = torch.from_numpy(coeffs[i, :count] / float(1 << 22))
    torch.manual_seed(1)
    w = torch.zeros(4, 3, 256, 256).uniform_(-.5, .5).requires_grad_(True)
    adam = torch.optim.Adam([w], lr=0.03)
    want_d, want_e = torch.tensor(D_FAKE_TARGETS), torch.tensor(ENTROPY_TARGETS)
    shift_d, shift_e = torch.zeros(4), torch.zeros(4)       # smooth score - true score, as last measured
    quantised = lambda: np.round(torch.tanh(w).detach().numpy() * LEVELS).astype(np.int8)
    for step in range(steps):
        disc, entr = smooth_scores(torch.tanh(w), netD, classifier, weights)
        if step % 20 == 0:
            true_d, true_e = host_scores(candidates(quantised()), netD, classifier, real)
            shift_d, shift_e = disc.detach() - torch.from_numpy(true_d).float(), entr.detach() - torch.from_numpy(true_e).float()
            print(step, np.round(true_d, 4), np.round(true_e, 4), flush=True)
        # Each score's slope with respect to the pattern, per candidate, scaled to length one (the entropy's is some hundred times the
        # flatter): a step goes down both, each counted in full until its score is within TOLERANCE of the target, then less and less
        slope_d, slope_e = torch.autograd.grad(disc.sum(), w, retain_graph=True)[0], torch.autograd.grad(entr.sum(), w)[0]
        unit = lambda g: g / g.flatten(1).norm(dim=1).clamp_min(1e-20).view(-1, 1, 1, 1)
        pull = lambda got, want, tol: torch.clamp((got.detach() - want) / tol, -1, 1).view(-1, 1, 1, 1)
        w.grad = (pull(disc - shift_d, want_d, TOLERANCE[0]) * unit(slope_d) + pull(entr - shift_e, want_e, TOLERANCE[1]) * unit(slope_e))
        for group in adam.param_groups:
            group["lr"] = 0.05 * min(1.0, 4.0 * (steps - step) / steps)      # full rate for three quarters, then down to nothing
        adam.step()
    levels = quantised()
    disc, entr = host_scores(candidates(levels), netD, classifier, real)
    gap_d, gap_e = np.diff(np.sort(disc)).min(), np.diff(np.sort(entr)).min()
    print("D_Fake", disc, "entropy", entr, "smallest gaps", gap_d, gap_e)
    assert gap_d >= 1.2e-2 and gap_e >= 1.05e-2, "the optimisation has not reached its targets: more steps"
    np.savez_compressed(out, levels=levels)


if __name__ == "__main__":
    main()
