"""GPU tests of best-of-N per view: the two kernels of libpixelsynth_rank_groups.so (csrc/rank_groups.hip) against their numpy
restatements bit for bit, get_best_sample(rank_scope="view") against the B = 1 device route of every view, forward_scene with B > 1 and
num_samples > 1 against every scene alone, and the driver's --num-samples."""
import functools
import itertools

import numpy as np
import pytest
import torch

from pixelsynth_amd import _lib, driver, ranking
from pixelsynth_amd import synthetic as syn
from rank_util import score_lists, select_cases
from test_rank_device_gpu import Spies, scorers, view  # noqa: F401  (the fixtures of the B = 1 device route: the same scorers, the same view)
from test_rank_groups_cpu import lay_out
from test_scene_batch_gpu import _one, _scene_batch, _scene_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = ranking.LAYOUTS


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---------------------------------------------------------------- ps_rank_select_groups
@functools.lru_cache(maxsize=None)
def group_lists(groups, n):
    """`groups` pairs of score lists of length n: rank_util.select_cases() of that n in turn (distinct scores; one NaN in either list),
    for n = 1024 the same made here"""
    cases = [c for c in select_cases() if len(c[0]) == n]
    if not cases:
        for seed in range(2):
            disc, entr = score_lists(n, seed)
            cases.append((disc, entr))
            for which in range(2):
                lists = [disc.copy(), entr.copy()]
                lists[which][(seed + 1) % n] = np.nan
                cases.append(tuple(lists))
    return [cases[g % len(cases)] for g in range(groups)]


SELECT_SHAPES = list(itertools.product((1, 3, 70), (1, 2, 17, 50, 64))) + [(2, 1024)]


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("groups,n", SELECT_SHAPES)
def test_select_groups_is_the_reference_in_every_group(groups, n, layout):
    per_group = group_lists(groups, n)
    disc, entr = lay_out(per_group, layout)
    want, want_d, want_e = ranking.select_groups_reference(disc, entr, groups, n, layout)
    best, disc_rank, entr_rank = ranking.select_groups(tt(disc), tt(entr), groups, n, layout, want_ranks=True)
    assert best.shape == (groups,) and best.dtype == torch.int32 and best.is_cuda
    assert np.array_equal(best.cpu().numpy(), want)
    assert np.array_equal(disc_rank.cpu().numpy(), want_d) and np.array_equal(entr_rank.cpu().numpy(), want_e)
    assert torch.equal(ranking.select_groups(tt(disc), tt(entr), groups, n, layout), best)           # (without the ranks; the same again)
    if groups == 1:
        one, one_d, one_e = ranking.select(tt(disc), tt(entr), want_ranks=True)
        assert int(one) == int(best[0]) and torch.equal(one_d, disc_rank) and torch.equal(one_e, entr_rank)
    else:   # the groups in another order: the results in that order
        perm = np.random.default_rng(groups * 1000 + n).permutation(groups)
        disc_p, entr_p = lay_out([per_group[g] for g in perm], layout)
        best_p, disc_rank_p, _ = ranking.select_groups(tt(disc_p), tt(entr_p), groups, n, layout, want_ranks=True)
        assert np.array_equal(best_p.cpu().numpy(), want[perm])
        gs, cs = ranking.group_strides(groups, n, layout)
        for k, g in enumerate(perm):
            at = np.arange(n) * cs
            assert np.array_equal(disc_rank_p.cpu().numpy()[k * gs + at], want_d[g * gs + at])


@pytest.mark.parametrize("layout", LAYOUTS)
def test_select_groups_resolves_equal_scores_to_the_lowest_index(layout):
    n = 17
    equal = (np.full(n, 0.25, np.float32), np.full(n, 2.0, np.float32))
    per_group = [group_lists(3, n)[0], equal, group_lists(3, n)[1]]
    disc, entr = lay_out(per_group, layout)
    best, disc_rank, entr_rank = ranking.select_groups(tt(disc), tt(entr), 3, n, layout, want_ranks=True)
    want, want_d, want_e = ranking.select_groups_reference(disc, entr, 3, n, layout)
    assert best.tolist() == list(want) and best[1] == 0
    assert np.array_equal(disc_rank.cpu().numpy(), want_d) and np.array_equal(entr_rank.cpu().numpy(), want_e)
    gs, cs = ranking.group_strides(3, n, layout)
    assert disc_rank.cpu().numpy()[gs + np.arange(n) * cs].tolist() == list(range(n))


def test_select_groups_refuses_what_it_does_not_take():
    scores = torch.zeros(64, device=DEV)
    best = torch.full((8,), -7, dtype=torch.int32, device=DEV)
    ranks = torch.full((64,), -7, dtype=torch.int32, device=DEV)
    for (groups, n, gs, cs), said in (((4, 4, 2, 4), r"strides \(group 2, candidate 4\)"), ((4, 4, 4, 4), "strides"), ((4, 4, 1, 1), "strides"),
                                      ((4, 0, 1, 4), "n = 0"), ((4, 1025, 1, 4), "n = 1025"), ((65536, 2, 1, 65536), "groups = 65536")):
        with pytest.raises(RuntimeError, match=r"ps_rank_select_groups failed \(rc=-\d+\): .*" + said):
            _lib.call("ps_rank_select_groups", scores, scores, groups, n, gs, cs, best, ranks, ranks)
    torch.cuda.synchronize()
    assert (best == -7).all() and (ranks == -7).all()
    for bad in (dict(groups=4, n=0), dict(groups=4, n=1025), dict(groups=65536, n=2), dict(groups=5, n=4)):
        with pytest.raises(ValueError, match="select_groups: expected two lists"):
            ranking.select_groups(scores[:16], scores[:16], **bad)
    with pytest.raises(ValueError, match="'row_major'"):
        ranking.select_groups(scores[:16], scores[:16], 4, 4, layout="row_major")


# ---------------------------------------------------------------- ps_rank_take_groups
def gather(src, best, groups, n, layout):
    gs, cs = ranking.group_strides(groups, n, layout)
    return src[np.arange(groups) * gs + np.clip(best, 0, n - 1) * cs]


GUARD = 8
TAKE_ITEMS = (1, 3, 4, 7, 1200, 4099, 8200)     # 4099, 8200: more than one chunk of an item per group, the last one partial, scalar and 16-byte


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("groups,n", [(1, 1), (1, 4), (5, 1), (5, 4)])
@pytest.mark.parametrize("item", TAKE_ITEMS)
def test_take_groups_is_the_numpy_gather_bit_for_bit(item, groups, n, layout):
    rng = np.random.default_rng(item * 100 + groups * 10 + n)
    src = rng.integers(0, 2 ** 32, (groups * n, item), dtype=np.uint32)        # any bit pattern, NaNs with payloads among them
    best = rng.integers(0, n, groups).astype(np.int32)
    want = gather(src, best, groups, n, layout)
    src_dev, best_dev = tt(src.view(np.int32)).view(torch.float32), tt(best)
    got = ranking.take_groups(src_dev, best_dev, n, layout)
    assert tuple(got.shape) == (groups, item) and got.dtype == torch.float32
    assert np.array_equal(got.view(torch.int32).cpu().numpy().view(np.uint32), want)
    gs, cs = ranking.group_strides(groups, n, layout)
    for offset in (0, 1):                    # out 16-byte aligned (torch's allocation), and one float further: the scalar path
        buf = torch.full((offset + groups * item + GUARD,), -7, dtype=torch.int32, device=DEV)
        out = buf[offset:offset + groups * item]
        assert out.data_ptr() % 16 == 4 * offset
        _lib.call("ps_rank_take_groups", src_dev, best_dev, groups, n, gs, cs, item, out)
        res = buf.cpu().numpy()
        assert np.array_equal(res[offset:offset + groups * item].view(np.uint32).reshape(groups, item), want), offset
        assert (res[:offset] == -7).all() and (res[offset + groups * item:] == -7).all(), offset
    if item == 4:                             # src one float further: the scalar path from the other side
        shifted = torch.empty(src_dev.numel() + 1, dtype=torch.float32, device=DEV)[1:].view(groups * n, item)
        shifted.view(torch.int32).copy_(src_dev.view(torch.int32))
        assert shifted.data_ptr() % 16 == 4
        assert torch.equal(ranking.take_groups(shifted, best_dev, n, layout).view(torch.int32), got.view(torch.int32))


@pytest.mark.parametrize("layout", LAYOUTS)
def test_take_groups_clamps_the_index_it_reads(layout):
    groups, n, item = 5, 4, 7
    src = np.random.default_rng(3).normal(size=(groups * n, item)).astype(np.float32)
    best = np.int32([-3, n + 2, 1, 2 ** 31 - 1, -2 ** 31])
    got = ranking.take_groups(tt(src), tt(best), n, layout).cpu().numpy()
    assert np.array_equal(got, gather(src, np.int32([0, n - 1, 1, n - 1, 0]), groups, n, layout))
    imgs = tt(src).view(groups * n, 7, 1)                               # the items keep their shape
    assert tuple(ranking.take_groups(imgs, tt(best), n, layout).shape) == (groups, 7, 1)
    with pytest.raises(ValueError, match="take_groups: expected groups"):
        ranking.take_groups(tt(src), tt(best[:3]), n, layout)
    with pytest.raises(ValueError, match="int32 index"):
        ranking.take_groups(tt(src), tt(best).long(), n, layout)


def test_score_candidates_in_chunks_is_the_single_pass(scorers, monkeypatch):
    """What the chunking itself decides -- which candidates a pass sees, and the order its scores come back in -- is checked exactly, on
    a stand-in pass.  On the real scorers a candidate's scores in chunks are within 1e-4 of the single pass: the project's allowance
    for the convolution library at another batch size, and between two calls at the same one (tests/test_rank_device_gpu.py; two
    calls of one pass on one batch are not the same bits, so nothing tighter is asked of them)."""
    netD, classifier = scorers
    cands = tt(syn.image(77, 5, 3, 256))
    disc, entr = ranking.score_candidates(cands, netD, classifier)
    for chunk in (2, 5, 64):
        disc_c, entr_c = ranking.score_candidates(cands, netD, classifier, chunk)
        assert disc_c.shape == entr_c.shape == (5,) and disc_c.is_cuda and entr_c.is_cuda
        err = float((disc - disc_c).abs().max()), float((entr - entr_c).abs().max())
        print(f"chunk {chunk}: max |single pass - chunks| D_Fake {err[0]:.3g}, entropy {err[1]:.3g}")
        assert max(err) <= 1e-4
    seen = []

    def one_pass(imgs, *scorers_):
        seen.append(imgs.shape[0])
        return imgs[:, 0, 0, 0].clone(), imgs[:, 1, 0, 0].clone()
    monkeypatch.setattr(ranking, "_score_pass", one_pass)
    for chunk, passes in ((None, [5]), (1, [1] * 5), (2, [2, 2, 1]), (4, [4, 1]), (5, [5]), (64, [5])):
        del seen[:]
        d, e = ranking.score_candidates(cands, netD, classifier, chunk)
        assert seen == passes, (chunk, seen)
        assert torch.equal(d, cands[:, 0, 0, 0]) and torch.equal(e, cands[:, 1, 0, 0]), chunk


# ---------------------------------------------------------------- get_best_sample(rank_scope="view")
N_VIEW = 3


@pytest.fixture(scope="module")
def three_views(view):
    """Three poses of the fixture's source: per view the B = 1 arguments of get_best_sample, and the same stacked to B = 3"""
    from pixelsynth_amd.z_buffermodel import build_ar_plan
    m, _, img, cam = view
    alone = []
    for direction in ("R", "L", "U"):
        RTinv, RT = m.get_rt_from_rot(direction, cam["P"])
        gen_fs, bg = m.pts_transformer.forward_justpts(img, syn.depth_from_image(img), cam["K"], cam["Kinv"], cam["P"], cam["Pinv"], RT, RTinv)
        alone.append((build_ar_plan(bg, 32), m.vqvae.encode_codes(gen_fs), bg, gen_fs))
    bg, gen_fs = torch.cat([a[2] for a in alone]), torch.cat([a[3] for a in alone])
    stacked = (build_ar_plan(bg, 32), torch.cat([a[1] for a in alone]), bg, gen_fs)
    assert not torch.equal(alone[0][2], alone[1][2]) and not torch.equal(alone[0][2], alone[2][2])
    return alone, stacked, img.expand(3, -1, -1, -1).contiguous()


@pytest.fixture
def three_samples(view, monkeypatch):
    monkeypatch.setattr(view[0].opt, "num_samples", N_VIEW)
    monkeypatch.delenv("PS_RANK", raising=False)
    monkeypatch.delenv("PS_RANK_SCOPE", raising=False)
    return view[0]


def test_get_best_sample_per_view_is_every_view_alone(scorers, view, three_views, three_samples, monkeypatch):
    netD, _ = scorers
    m, img = three_samples, view[2]
    alone, stacked, img3 = three_views
    B, n = 3, N_VIEW
    spies = Spies(monkeypatch, m, netD)
    best = m.get_best_sample(*stacked, netD, img3, rank_scope="view")
    # (d) nothing per candidate, nothing through the host: one batched scoring of the n * B candidates
    assert not spies.per_candidate and len(spies.batched) == 1 and len(spies.decoded) == n
    assert all(tuple(c.shape) == (B, 3, 256, 256) for c in spies.decoded) and tuple(best.shape) == (B, 3, 256, 256)
    decoded = list(spies.decoded)
    disc, entr = (s.cpu().numpy() for s in spies.batched[0])
    assert disc.shape == entr.shape == (n * B,) and np.isfinite(disc).all() and np.isfinite(entr).all()
    want, _, _ = ranking.select_groups_reference(disc, entr, B, n)
    for b in range(B):
        m.get_best_sample(*alone[b], netD, img, rank_on="device")
        assert not spies.per_candidate and len(spies.batched) == 2 + b and len(spies.decoded) == n * (2 + b)
        own_disc, own_entr = (s.cpu().numpy() for s in spies.batched[1 + b])
        for i in range(n):
            cand = spies.decoded[n * (1 + b) + i]
            # (a) the candidate of the batch is the candidate of the view alone
            assert torch.equal(decoded[i][b:b + 1], cand), f"view {b} candidate {i}: max |d| = {(decoded[i][b:b + 1] - cand).abs().max().item():.3g}"
            # (b) and scores alike
            err = abs(disc[i * B + b] - own_disc[i]), abs(entr[i * B + b] - own_entr[i])
            print(f"view {b} candidate {i}: |batched - alone| D_Fake {err[0]:.3g}, entropy {err[1]:.3g}")
            assert max(err) <= 1e-4
        # (c) the view's slice of the result is the candidate the rule keeps on the batched scores
        assert torch.equal(best[b], decoded[want[b]][b]), b
    assert not torch.equal(decoded[0][0], decoded[1][0]) and not torch.equal(decoded[0][0], decoded[0][1])
    # the option and the variable select the route as the argument does: the same candidates, every view's winner by that run's own
    # scores (two runs' scores differ by the convolution library's noise, which may flip a near-tie)
    def again(**kw):
        got = m.get_best_sample(*stacked, netD, img3, **kw)
        assert not spies.per_candidate and all(torch.equal(a, c) for a, c in zip(decoded, spies.decoded[-n:]))
        keep, _, _ = ranking.select_groups_reference(*(s.cpu().numpy() for s in spies.batched[-1]), B, n)
        assert all(torch.equal(got[b], decoded[keep[b]][b]) for b in range(B))
    monkeypatch.setattr(m.opt, "rank_scope", "view", raising=False)
    again()
    assert len(spies.batched) == 2 + B
    monkeypatch.delattr(m.opt, "rank_scope")
    monkeypatch.setenv("PS_RANK_SCOPE", "view")
    again(rank_on="device")
    assert len(spies.batched) == 3 + B


def test_get_best_sample_batch_scope_and_default_stay_as_they_are(scorers, view, three_views, monkeypatch):
    """(e) unset, "batch", and "view" at B = 1: the calls of test_get_best_sample_unset_stays_on_the_host_route; "batch" at B = 3: the
    host route's one winner index for the whole batch"""
    netD, _ = scorers
    m, args, img, _ = view
    alone, stacked, img3 = three_views
    monkeypatch.delenv("PS_RANK", raising=False)
    monkeypatch.delenv("PS_RANK_SCOPE", raising=False)
    spies = Spies(monkeypatch, m, netD)
    m.get_best_sample(*args, netD, img)
    assert spies.per_candidate == ["disc", "entr"] * 4 and not spies.batched and len(spies.decoded) == 4
    first = list(spies.decoded)
    for k, scope in enumerate(("batch", "view")):
        m.get_best_sample(*args, netD, img, rank_scope=scope)
        assert spies.per_candidate == ["disc", "entr"] * 4 * (k + 2) and not spies.batched and len(spies.decoded) == 4 * (k + 2)
        assert all(torch.equal(a, b) for a, b in zip(first, spies.decoded[4 * (k + 1):]))
    monkeypatch.setattr(m.opt, "num_samples", N_VIEW)
    del spies.per_candidate[:], spies.decoded[:]
    best = m.get_best_sample(*stacked, netD, img3, rank_scope="batch")
    assert spies.per_candidate == ["disc", "entr"] * N_VIEW and not spies.batched and len(spies.decoded) == N_VIEW
    assert any(torch.equal(best, c) for c in spies.decoded)                  # one candidate index for all three views
    decoded = list(spies.decoded)
    unset = m.get_best_sample(*stacked, netD, img3)                          # unset: the same calls, the same candidates (the winner
    assert spies.per_candidate == ["disc", "entr"] * N_VIEW * 2 and not spies.batched      # is each run's own: two runs' host scores
    assert all(torch.equal(a, b) for a, b in zip(decoded, spies.decoded[N_VIEW:]))         # differ by the convolution library's noise,
    assert any(torch.equal(unset, c) for c in decoded)                                     # which may flip a near-tie)


def test_get_best_sample_per_view_refuses_what_it_cannot_do(scorers, view, three_views, three_samples, monkeypatch):
    netD, _ = scorers
    m = three_samples
    _, stacked, img3 = three_views
    with pytest.raises(ValueError, match="shard"):                                                    # (g)
        m.get_best_sample(*stacked, netD, img3, rank_scope="view", shard=True)
    with pytest.raises(NotImplementedError, match="num_samples.*can_score_on_device"):
        m.get_best_sample(*stacked, netD, img3, rank_scope="view", rank_on="host")
    with pytest.raises(ValueError, match="'scene'"):
        m.get_best_sample(*stacked, netD, img3, rank_scope="scene")

    class D:   # the stand-ins of test_get_best_sample_falls_back_for_stand_in_scorers
        def run_discriminator_one_step(self, fake, real):
            raise AssertionError("the per-view route has no host side")

    class C(torch.nn.Module):
        def forward(self, x):
            raise AssertionError("the per-view route has no host side")
    spies = Spies(monkeypatch, m, None)
    with pytest.raises(NotImplementedError, match="num_samples.*can_score_on_device"):               # (f)
        m.get_best_sample(*stacked, D(), img3, rank_scope="view")
    monkeypatch.setattr(m, "classifier", C())
    with pytest.raises(NotImplementedError, match="num_samples"):
        m.get_best_sample(*stacked, D(), img3, rank_scope="view", rank_on="device")
    assert not spies.decoded and not spies.batched and not spies.per_candidate


# ---------------------------------------------------------------- forward_scene, B > 1 and num_samples > 1
def test_forward_scene_batch_ranks_every_scene_as_the_scene_alone(scorers, monkeypatch):
    """gen_scene, directions R, num_split 2, three candidates per frame, two scenes.  Every frame's winner indices are recorded; every
    scene then runs alone on the B = 1 device route with ranking.select handing back the recorded index of that frame and scene, so
    that the comparison does not hang on a near-tie that another batch size could flip: every output is the batch's slice bit for bit,
    the scores agree within 1e-4, and each recorded index is the rule's choice on the batched scores."""
    netD, classifier = scorers
    B, n = 2, 3
    m = _scene_model(directions=["R"], num_split=2)
    m.classifier = classifier
    m.opt.num_samples = n
    monkeypatch.delenv("PS_RANK", raising=False)
    monkeypatch.delenv("PS_RANK_SCOPE", raising=False)
    frames = []
    inner = ranking.select_groups

    def select_groups(disc, entr, groups, count, *a, **kw):
        best = inner(disc, entr, groups, count, *a, **kw)
        frames.append((disc.cpu().numpy(), entr.cpu().numpy(), best.cpu().tolist()))
        assert (groups, count) == (B, n) and not a and not kw
        return best
    monkeypatch.setattr(ranking, "select_groups", select_groups)
    batch = _scene_batch(B)
    _, out = m(batch, netD)
    m.outpaint2.engine(32, 32, B).check()
    assert len(frames) == 3 and tuple(out["PredImg_R_0"].shape) == (B, 3, 256, 256)
    for disc, entr, best in frames:
        for b in range(B):
            assert best[b] == ranking.select_reference(disc[b::B], entr[b::B])[0]
    monkeypatch.setattr(m.opt, "rank_on", "device", raising=False)
    flipped = 0
    for b in range(B):
        own = []

        def select(disc, entr, want_ranks=False):
            own.append((disc.cpu().numpy(), entr.cpu().numpy()))
            return torch.tensor([frames[len(own) - 1][2][b]], device=disc.device)
        monkeypatch.setattr(ranking, "select", select)
        _, one = m(_one(batch, b), netD)
        m.outpaint2.engine(32, 32, 1).check()
        assert len(own) == len(frames)
        for f, (disc, entr) in enumerate(own):
            err = np.abs(disc - frames[f][0][b::B]).max(), np.abs(entr - frames[f][1][b::B]).max()
            print(f"scene {b} frame {f}: |alone - batched| D_Fake {err[0]:.3g}, entropy {err[1]:.3g}")
            assert max(err) <= 1e-4
            flipped += ranking.select_reference(disc, entr)[0] != frames[f][2][b]
        assert set(one) <= set(out)
        for k, v in one.items():
            assert torch.equal(out[k][b:b + 1], v), f"scene {b}: {k}, max |d| = {(out[k][b:b + 1].float() - v.float()).abs().max().item():.3g}"
    print(f"{flipped} of {B * len(frames)} frames: the unforced rule on the scene's own scores chooses another candidate")
    winners = [best for _, _, best in frames]
    print("winner indices per frame:", winners)


# ---------------------------------------------------------------- the driver
def test_driver_renders_scenes_with_num_samples(scorers, tmp_path):
    netD, classifier = scorers
    paths = []
    for i in range(2):
        paths.append(str(tmp_path / f"src{i}.png"))
        driver.save_png(paths[-1], torch.from_numpy(syn.image(50 + i, 1, 3, 256))[0])
    torch.save(netD.state_dict(), str(tmp_path / "netD.pt"))
    torch.save(classifier.state_dict(), str(tmp_path / "classifier.pt"))
    argv = ["--image", *paths, "--scene", "R", "--num-split", "1", "--batch", "2", "--num-samples", "2", "--out", str(tmp_path / "out"),
            "--discriminator", str(tmp_path / "netD.pt")]
    with pytest.raises(SystemExit) as exit_:
        driver.main(argv)
    assert exit_.value.code == 2 and not (tmp_path / "out").exists()
    driver.main(argv + ["--classifier", str(tmp_path / "classifier.pt")])
    for scene in ("0000", "0001"):
        folder = tmp_path / "out" / scene
        assert (folder / "scene" / "output_image_R_0001.png").is_file()
        assert sorted(p.name for p in (folder / "video").iterdir()) == ["0.png", "1.png"]
