"""GPU tests of the device ranking route: the four passes of libpixelsynth_rank.so (csrc/rank.hip) against Pillow, fp64 and the host
route's own formulas, both routes on the real scorer mirrors, and get_best_sample(rank_on="device")."""
import argparse
import functools
import math
import os
import types

import numpy as np
import pytest
import torch

from pixelsynth_amd import ranking
from pixelsynth_amd import synthetic as syn
from pixelsynth_amd.z_buffermodel import rank_samples
from rank_util import SIZES, host_lines, input_images, select_cases

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------- ps_rank_classifier_input
@functools.lru_cache(maxsize=None)
def input_case(S, T):
    """The kernel's inputs and what the host makes of them, once per shape: Pillow's bytes, the restatement's fp32"""
    imgs = input_images(S)
    want, want_bytes = ranking.classifier_input_reference(imgs, T)
    pillow = np.stack([host_lines(im, T)[1] for im in imgs])
    return imgs, want, want_bytes, pillow


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("S,T", SIZES)
def test_classifier_input_is_the_host_route_bit_for_bit(S, T, N):
    """uint8 output == Pillow, fp32 output == the restatement (which the CPU tests pin to _entropy_score's lines); every image alone
    (N = 1) and the three in one batch: a candidate's result does not depend on its place."""
    imgs, want, want_bytes, pillow = input_case(S, T)
    assert np.array_equal(want_bytes, pillow)
    for sel in ([slice(0, 3)] if N == 3 else [slice(i, i + 1) for i in range(3)]):
        out, resized = ranking.classifier_input(tt(imgs[sel]), T, want_bytes=True)
        assert out.shape == (sel.stop - sel.start, 3, T, T) and resized.dtype == torch.uint8
        assert np.array_equal(resized.cpu().numpy(), pillow[sel])
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want[sel].view(np.uint32))
        assert torch.equal(ranking.classifier_input(tt(imgs[sel]), T), out)        # (without the bytes; and the same bits again)


def test_classifier_input_outside_the_range_is_what_the_header_defines():
    x = np.zeros((1, 3, 16, 16), np.float32)
    x.reshape(-1)[:8] = [3.0, -3.0, 1e30, -1e30, np.nan, np.inf, -np.inf, 1.5]
    want, want_bytes = ranking.classifier_input_reference(x, 16)
    out, resized = ranking.classifier_input(tt(x), 16, want_bytes=True)
    assert np.array_equal(resized.cpu().numpy(), want_bytes) and np.array_equal(out.cpu().numpy(), want)
    assert list(want_bytes.reshape(-1)[:8]) == [254, 1, 128, 0, 0, 128, 0, 62]      # (16 -> 16: the resample is the identity)


# ---------------------------------------------------------------- ps_rank_entropy
def host_entropy(logits):
    """_entropy_score's last lines on one row of logits (a CPU fp32 tensor)"""
    probs = torch.softmax(logits[None].float().cpu(), 1).squeeze(0).numpy()
    probs = np.sort(probs)[::-1]
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(-np.sum(probs * np.log(probs)))


@pytest.mark.parametrize("N", [1, 5])
@pytest.mark.parametrize("C", [1, 2, 10, 365, 1000])
def test_entropy_against_fp64_and_the_host_formula(C, N):
    """|device - fp64 on the same fp32 logits| <= 2e-5: sum |p log p| <= ln 1000 = 6.9, a few ulp (6e-8 each) per term from exp, log and
    the division, a serial partial sum of <= 16 terms per lane and a 6-level butterfly.  Within 1e-4 of the host formula."""
    logits = torch.from_numpy(np.random.default_rng(C * 10 + N).normal(0, 3, (N, C)).astype(np.float32))
    got = ranking.entropy(logits.to(DEV)).cpu().numpy()
    p = torch.softmax(logits.double(), 1)
    want = -(p * torch.log(p)).sum(1).numpy()
    err = np.abs(got - want).max()
    print(f"entropy C={C} N={N}: max |device - fp64| = {err:.3g}")
    assert got.dtype == np.float32 and err <= 2e-5
    assert max(abs(got[n] - host_entropy(logits[n])) for n in range(N)) <= 1e-4
    flat = ranking.entropy(torch.full((N, C), 1.25, device=DEV)).cpu().numpy()
    assert np.abs(flat - math.log(C)).max() <= 2e-5


def test_entropy_keeps_the_nan_of_an_underflowed_class():
    """exp(-200) is 0 in fp32: 0 * log 0 = NaN on the host route (numpy's probs * log(probs)), and here"""
    logits = torch.zeros(3, 10)
    logits[1, 4] = 200.0
    got = ranking.entropy(logits.to(DEV)).cpu().numpy()
    assert math.isnan(host_entropy(logits[1])) and math.isnan(got[1])
    assert abs(got[0] - math.log(10)) <= 2e-5 and got[0] == got[2]


# ---------------------------------------------------------------- ps_rank_hinge_fake
@pytest.mark.parametrize("shape0,shape1", [((35, 35), (19, 19)), ((1, 1), (1, 1)), ((3, 5), (2, 2))])
def test_hinge_fake_against_fp64_and_ganloss(shape0, shape1):
    """<= 2e-6 * max(1, mean |term|) from fp64 (the terms are rounded to fp32 once, 6e-8 relative; the sums are carried in fp64 and
    rounded once more), <= 1e-6 from GANLoss applied to each sample alone."""
    from pixelsynth_amd.losses.gan_loss import GANLoss
    rng = np.random.default_rng(shape0[0])
    N = 4
    maps = [rng.normal(-0.5, 1.0, (N, 1) + s).astype(np.float32) for s in (shape0, shape1)]
    one = np.float32(-1.0)
    edge = [one, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(-2))]    # the hinge's corner and either side of it
    for n in range(N):
        for m in maps:
            m[n].reshape(-1)[:len(edge)] = np.roll(edge, n)[:m[n].size]
    got = ranking.hinge_fake(tt(maps[0]), tt(maps[1])).cpu().numpy()
    crit = GANLoss("hinge")
    for n in range(N):
        terms = [np.minimum(-m[n].astype(np.float64) - 1.0, 0.0) for m in maps]
        want = 0.5 * sum(-t.mean() for t in terms)
        scale = max(1.0, 0.5 * sum(np.abs(t).mean() for t in terms))
        alone = float(crit([[torch.from_numpy(m[n:n + 1])] for m in maps], False, for_discriminator=True))
        print(f"hinge {shape0} {shape1} n={n}: |device - fp64| = {abs(got[n] - want):.3g}, |device - GANLoss| = {abs(got[n] - alone):.3g}")
        assert abs(got[n] - want) <= 2e-6 * scale and abs(got[n] - alone) <= 1e-6
    again = ranking.hinge_fake(tt(maps[0][1:2]), tt(maps[1][1:2])).cpu().numpy()
    assert again[0] == got[1]                                                       # (alone or in the batch: the same bits)


# ---------------------------------------------------------------- ps_rank_select
def test_select_is_rank_samples_and_the_reference():
    for disc, entr in select_cases():
        best, disc_rank, entr_rank = ranking.select(tt(disc), tt(entr), want_ranks=True)
        want, want_d, want_e = ranking.select_reference(disc, entr)
        assert best.shape == (1,) and best.dtype == torch.int64
        assert int(best) == want == rank_samples(disc, entr) == int(ranking.select(tt(disc), tt(entr)))
        assert np.array_equal(disc_rank.cpu().numpy(), want_d) and np.array_equal(entr_rank.cpu().numpy(), want_e)
    big = np.random.default_rng(0).normal(size=(2, 1024)).astype(np.float32)             # the largest n, every thread with four elements
    assert int(ranking.select(tt(big[0]), tt(big[1]))) == ranking.select_reference(big[0], big[1])[0]


def test_select_resolves_equal_scores_to_the_lower_index():
    disc, entr = np.float32([1.0, 1.0, 0.0]), np.float32([2.0, 2.0, 2.0])
    best, disc_rank, entr_rank = ranking.select(tt(disc), tt(entr), want_ranks=True)
    assert disc_rank.tolist() == [1, 2, 0] and entr_rank.tolist() == [0, 1, 2] and int(best) == 0    # totals 3, 3, 0
    best, disc_rank, _ = ranking.select(tt(np.float32([0.5, -0.0, 0.0, np.nan, np.nan])), tt(np.float32([5, 4, 3, 2, 1])), want_ranks=True)
    assert disc_rank.tolist() == [2, 0, 1, 3, 4] and int(best) == 4


# ---------------------------------------------------------------- the two scorers, both routes
@pytest.fixture(scope="module")
def scorers():
    """The weights of test_get_best_sample_runs_end_to_end_with_the_real_scorers: the discriminator mirror filled by
    fill_state_dict(shapes, 9), the ResNet-18 as torch.manual_seed(0) initialises it"""
    from pixelsynth_amd.losses import DiscriminatorLoss
    from pixelsynth_amd.networks import resnet18
    torch.manual_seed(0)
    classifier = resnet18(num_classes=365).eval().to(DEV)
    opt = argparse.Namespace(discriminator_losses="pix2pixHD", gan_mode="hinge", norm_D="spectralinstance", ndf=64, output_nc=3,
                             no_ganFeat_loss=False, isTrain=False, lambda_feat=10.0)
    netD = DiscriminatorLoss(opt).eval()
    shapes = {k: tuple(v.shape) for k, v in netD.state_dict().items()}
    netD.load_state_dict({k: torch.from_numpy(v) for k, v in syn.fill_state_dict(shapes, 9).items()}, strict=True)
    return netD.to(DEV), classifier


def test_both_routes_score_the_real_mirrors_alike(scorers):
    """Four fixed candidates (tests/golden/rank_candidates.npz, made by make_rank_candidates.py: patterns in [-1,1] chosen so that the
    HOST route's scores are at least 1e-2 apart in both lists -- a condition of this test, asserted).  Each score agrees within 1e-4
    (the project's allowance for the convolution library choosing another algorithm at another batch size), the winner is the same."""
    from pixelsynth_amd.z_buffermodel import ZbufferModelPts
    netD, classifier = scorers
    levels = np.load(os.path.join(GOLDEN, "rank_candidates.npz"))["levels"]
    assert levels.dtype == np.int8 and levels.shape == (4, 3, 256, 256) and np.abs(levels).max() <= 7
    cands = tt(levels.astype(np.float32) / np.float32(7))                           # in [-1,1], fifteen levels
    real = tt(syn.image(31, 1, 3, 256))
    holder = type("H", (), {"classifier": classifier, "_entropy_score": ZbufferModelPts._entropy_score})()
    with torch.no_grad():
        disc = [float(netD.run_discriminator_one_step(cands[i:i + 1], real)["D_Fake"].mean().cpu()) for i in range(4)]
        entr = [holder._entropy_score(cands[i:i + 1]) for i in range(4)]
    gaps = np.diff(np.sort(disc)).min(), np.diff(np.sort(entr)).min()
    print("host D_Fake", disc, "entropy", entr, "smallest gaps", gaps)
    assert min(gaps) >= 1e-2, "the candidates do not hold the host scores apart"
    disc_dev, entr_dev = ranking.score_candidates(cands, netD, classifier)
    assert disc_dev.is_cuda and entr_dev.is_cuda and disc_dev.shape == entr_dev.shape == (4,)
    err = np.abs(disc_dev.cpu().numpy() - disc).max(), np.abs(entr_dev.cpu().numpy() - entr).max()
    print("max |device - host|: D_Fake %.3g, entropy %.3g" % err)
    assert max(err) <= 1e-4
    assert int(ranking.select(disc_dev, entr_dev)) == rank_samples(disc, entr)


# ---------------------------------------------------------------- get_best_sample(rank_on="device")
@pytest.fixture(scope="module")
def view(scorers):
    """A model with num_samples = 4 and the view of the existing end-to-end test, the model's classifier the fixture's"""
    from pixelsynth_amd.z_buffermodel import ZbufferModelPts, build_ar_plan
    o = dict(W=256, use_rgb_features=True, splatter="xyblending", learn_default_feature=True, radius=4, pp_pixel=128, tau=1.0,
             rad_pow=2, accumulation="alphacomposite", background_smoothing_kernel_size=13, min_z=1.0, max_z=100.0, rotation=0.6,
             direction="R", temperature=0.7, model_setting="gen_img", seed=0, homography=False, vqvae=True, num_samples=4)
    m = ZbufferModelPts(types.SimpleNamespace(**o), classifier=scorers[1]).eval()
    m.outpaint2.load_state_dict({k: torch.from_numpy(v) for k, v in syn.pixelcnn_state_dict(0).items()})
    m.vqvae.load_state_dict({k: torch.from_numpy(v) for k, v in syn.vqvae_state_dict(0).items()}, strict=True)
    m = m.to(DEV).eval()
    img = tt(syn.image(31, 1, 3, 256))
    cam = {k: tt(v) for k, v in syn.demo_cameras(1).items()}
    RTinv, RT = m.get_rt_from_rot("R", cam["P"])
    gen_fs, bg = m.pts_transformer.forward_justpts(img, syn.depth_from_image(img), cam["K"], cam["Kinv"], cam["P"], cam["Pinv"], RT, RTinv)
    return m, (build_ar_plan(bg, 32), m.vqvae.encode_codes(gen_fs), bg, gen_fs), img, cam


class Spies:
    """Counts the per-candidate scorers of the host route and the batched one of the device route, records every decoded candidate"""

    def __init__(self, monkeypatch, m, netD):
        self.per_candidate, self.batched, self.decoded = [], [], []
        inner_d = getattr(netD, "run_discriminator_one_step", None)     # (netD None: the test's own stand-in counts for itself)
        inner_e, inner_c, inner_s = m._entropy_score, m._decode_checked, ranking.score_candidates

        def disc(fake, real):
            self.per_candidate.append("disc")
            return inner_d(fake, real)

        def entr(img):
            self.per_candidate.append("entr")
            return inner_e(img)

        def decode(*a, **kw):
            self.decoded.append(inner_c(*a, **kw))
            return self.decoded[-1]

        def score(*a):
            self.batched.append(inner_s(*a))
            return self.batched[-1]
        if netD is not None:
            monkeypatch.setattr(netD, "run_discriminator_one_step", disc, raising=False)
        monkeypatch.setattr(m, "_entropy_score", entr, raising=False)
        monkeypatch.setattr(m, "_decode_checked", decode, raising=False)
        monkeypatch.setattr(ranking, "score_candidates", score)


def test_get_best_sample_on_the_device_route(scorers, view, monkeypatch):
    netD, _ = scorers
    m, args, img, cam = view
    monkeypatch.delenv("PS_RANK", raising=False)
    spies = Spies(monkeypatch, m, netD)
    best = m.get_best_sample(*args, netD, img, rank_on="device")
    assert not spies.per_candidate and len(spies.batched) == 1 and len(spies.decoded) == 4
    assert all(tuple(c.shape) == (1, 3, 256, 256) for c in spies.decoded) and not torch.equal(spies.decoded[0], spies.decoded[1])
    disc, entr = spies.batched[0]
    assert torch.isfinite(disc).all() and torch.isfinite(entr).all()
    assert torch.equal(best, spies.decoded[int(ranking.select(disc, entr))])
    # the reference-shaped entry point hands the option on; the model's own option does the same
    batch = {"images": [img.cpu()], "cameras": [{k: v.cpu() for k, v in cam.items()}], "depths": [syn.depth_from_image(img).cpu()]}
    _, out = m.forward_image(batch, netD=netD, rank_on="device")
    assert not spies.per_candidate and len(spies.batched) == 2 and len(spies.decoded) == 8
    assert torch.equal(out["PredImg"], spies.decoded[4 + int(ranking.select(*spies.batched[1]))])
    with pytest.raises(ValueError, match="'gpu'"):
        m.get_best_sample(*args, netD, img, rank_on="gpu")


def test_get_best_sample_unset_stays_on_the_host_route(scorers, view, monkeypatch):
    netD, _ = scorers
    m, args, img, _ = view
    monkeypatch.delenv("PS_RANK", raising=False)
    spies = Spies(monkeypatch, m, netD)
    m.get_best_sample(*args, netD, img)
    assert spies.per_candidate == ["disc", "entr"] * 4 and not spies.batched and len(spies.decoded) == 4
    decoded = list(spies.decoded)
    monkeypatch.setattr(m.opt, "rank_on", "device", raising=False)                      # the option, where the argument is not given
    best = m.get_best_sample(*args, netD, img)
    assert len(spies.per_candidate) == 8 and len(spies.batched) == 1
    assert all(torch.equal(a, b) for a, b in zip(decoded, spies.decoded[4:]))          # both routes decode the same candidates
    assert torch.equal(best, decoded[int(ranking.select(*spies.batched[0]))])


def test_get_best_sample_falls_back_for_stand_in_scorers(view, monkeypatch):
    m, args, img, _ = view
    seen = []

    class D:   # the stand-ins of test_get_best_sample_ranks_candidates
        def run_discriminator_one_step(self, fake, real):
            seen.append(fake)
            return {"D_Fake": fake.mean().reshape(1)}

    class C(torch.nn.Module):
        def forward(self, x):
            return torch.cat([x.mean().reshape(1, 1) * k for k in range(1, 11)], 1)
    monkeypatch.setattr(m, "classifier", C())
    spies = Spies(monkeypatch, m, None)
    best = m.get_best_sample(*args, D(), img, rank_on="device")
    assert len(seen) == 4 and spies.per_candidate == ["entr"] * 4 and not spies.batched
    monkeypatch.undo()
    monkeypatch.setattr(m, "classifier", C())
    assert torch.equal(best, seen[rank_samples([float(s.mean()) for s in seen], [m._entropy_score(s) for s in seen])])


def test_get_best_sample_shard_downloads_its_scores_once(scorers, view, monkeypatch):
    """shard=True on the device route, as rank 0 of two (the collectives replaced by stand-ins): candidates 0 and 2 are scored in one
    batch, their two vectors reach gather_scores, and the host rule does the rest"""
    from pixelsynth_amd import distributed as D
    netD, _ = scorers
    m, args, img, _ = view
    spies = Spies(monkeypatch, m, netD)
    handed = []

    def gather(disc, entr, n):
        handed.append((list(disc), list(entr)))
        d_all, e_all = np.full(n, -1e9), np.full(n, 1e9)      # the other rank's candidates lose in both lists
        d_all[0::2], e_all[0::2] = disc, entr
        return d_all, e_all
    monkeypatch.setattr(D, "world", lambda: (0, 2))
    monkeypatch.setattr(D, "gather_scores", gather)
    monkeypatch.setattr(D, "broadcast_from", lambda tensor, src, device: tensor)
    best = m.get_best_sample(*args, netD, img, shard=True, rank_on="device")
    assert not spies.per_candidate and len(spies.batched) == 1 and len(spies.decoded) == 2 and len(handed) == 1
    disc, entr = spies.batched[0]
    assert handed[0] == (disc.double().cpu().tolist(), entr.double().cpu().tolist())
    assert torch.equal(best, spies.decoded[int(ranking.select(disc, entr))])


# ---------------------------------------------------------------- the candidates: when they are decoded, how they are grouped
def test_host_route_scores_a_candidate_before_the_next_is_decoded(scorers, view, monkeypatch):
    """Two candidates per engine run: a candidate still goes through the discriminator and the classifier before the next one is
    decoded -- one log fed by all three reads decode, disc, entr four times over"""
    netD, _ = scorers
    m, args, img, _ = view
    monkeypatch.delenv("PS_RANK", raising=False)
    monkeypatch.setattr(m, "sample_batch", 2)
    log = []

    def logged(name, inner):
        def spy(*a, **kw):
            log.append(name)
            return inner(*a, **kw)
        return spy
    monkeypatch.setattr(m, "_decode_checked", logged("decode", m._decode_checked), raising=False)
    monkeypatch.setattr(netD, "run_discriminator_one_step", logged("disc", netD.run_discriminator_one_step), raising=False)
    monkeypatch.setattr(m, "_entropy_score", logged("entr", m._entropy_score), raising=False)
    m.get_best_sample(*args, netD, img, rank_on="host")
    assert log == ["decode", "disc", "entr"] * 4


def test_grouping_of_the_engine_runs_does_not_matter(scorers, view, monkeypatch):
    """sample_batch 1, 2 and 32 -- four engine runs of one frame, two of two, one of four -- with the same draws: the same decoded
    candidates, bit for bit, and the same winner, on both routes.
    The winner is compared from run to run, so it must not hang on the last bit of a score: the classifier of the fixture is a random
    initialisation, its entropies of the four candidates lie within 1e-6 of one another, and the same candidate's entropy differs by
    5e-7 between two calls of the same code (measured: the classifier's kernels do not sum in a fixed order) -- so on both routes the
    entropy is replaced by a quantity that separates the candidates and has a fixed summation order, the fp64 sum of the image.  The
    discriminator's scores stay -- they move by one ulp, 6e-8, between two calls at the most (measured), and lie 1e-6 apart and more: a
    condition of this test, asserted -- and so does the rank rule of either route."""
    netD, _ = scorers
    m, args, img, _ = view
    monkeypatch.delenv("PS_RANK", raising=False)
    uniforms = torch.rand(4, 1, 1024, generator=torch.Generator(device="cpu").manual_seed(7)).to(DEV)
    score_candidates = ranking.score_candidates
    monkeypatch.setattr(m, "_entropy_score", lambda im: float(im.double().sum().cpu()), raising=False)
    monkeypatch.setattr(ranking, "score_candidates", lambda stack, *a: (score_candidates(stack, *a)[0], stack.double().sum((1, 2, 3)).float()))
    for route in ("host", "device"):
        runs = []
        for per_run in (1, 2, 32):
            with monkeypatch.context() as mp:
                mp.setattr(m, "sample_batch", per_run)
                spies = Spies(mp, m, netD)
                best = m.get_best_sample(*args, netD, img, uniforms=uniforms, rank_on=route)
            assert len(spies.decoded) == 4 and len(spies.batched) == (route == "device")
            assert spies.per_candidate == ([] if route == "device" else ["disc", "entr"] * 4)
            if route == "device":
                gap = float(spies.batched[0][0].sort().values.diff().min())
                print(f"sample_batch {per_run}: smallest gap between two candidates' D_Fake {gap:.3g}")
                assert gap >= 1e-6, "the candidates do not hold the discriminator's scores apart"
            runs.append((spies.decoded, best))
        for decoded, best in runs[1:]:
            assert all(torch.equal(a, b) for a, b in zip(runs[0][0], decoded)), route
            assert torch.equal(best, runs[0][1]), route
        assert any(torch.equal(runs[0][1], c) for c in runs[0][0]), route             # (the winner is one of the four)
