"""CPU-only: the host side of the device ranking route (pixelsynth_amd/ranking.py) -- the numpy restatement of the classifier's input
against Pillow and against _entropy_score's own lines, the rank rule against rank_samples, the C ABI of libpixelsynth_rank.so against its
header and bindings, and what decides between the two routes of get_best_sample."""
import argparse

import numpy as np
import pytest
import torch
from PIL import Image

from abi_util import assert_library_matches_header
from pixelsynth_amd import _lib, _libraries, ranking
from pixelsynth_amd.z_buffermodel import _rank_route, rank_samples
from rank_util import SIZES, byte_images, floats_of_bytes, host_lines, score_lists


@pytest.mark.parametrize("S,T", SIZES)
def test_the_resample_restatement_is_pillow_bit_for_bit(S, T):
    for name, raw in byte_images(S).items():
        want = np.asarray(Image.fromarray(raw).resize((T, T), Image.BILINEAR))
        assert np.array_equal(ranking.resize_reference(raw, T), want), name
        # and through the whole restatement: the floats are READ AS (S,S,3), so the candidate is that picture's bytes laid out flat
        out, resized = ranking.classifier_input_reference(floats_of_bytes(raw).reshape(1, 3, S, S), T)
        assert resized.dtype == np.uint8 and np.array_equal(resized[0], want), name


@pytest.mark.parametrize("S,T", SIZES)
def test_the_restatement_is_the_entropy_scores_own_lines(S, T):
    rng = np.random.default_rng(S * 1000 + T)
    imgs = rng.uniform(-1, 1, (2, 3, S, S)).astype(np.float32)
    imgs[0, 0, 0, :4] = [1.0, -1.0, 0.0, -0.0]
    out, resized = ranking.classifier_input_reference(imgs, T)
    assert out.dtype == np.float32 and out.shape == (2, 3, T, T)
    for n in range(2):
        want, want_bytes = host_lines(imgs[n], T)
        assert np.array_equal(resized[n], want_bytes)
        assert np.array_equal(out[n].view(np.uint32), want.view(np.uint32))


def test_the_tables_of_256_to_224():
    bounds, coeffs = ranking.pil_bilinear_tables(256, 224)
    assert bounds.shape == (224, 2) and coeffs.shape == (224, 5) and bounds.dtype == coeffs.dtype == np.int32
    assert set(bounds[:, 1]) == {2, 3} and bounds[0, 0] == 0 and bounds[-1].sum() == 256
    assert np.all(np.diff(bounds[:, 0]) >= 0) and np.all(np.abs(coeffs.sum(1) - (1 << 22)) <= 2)
    assert all(np.all(coeffs[i, c:] == 0) for i, c in enumerate(bounds[:, 1]))
    with pytest.raises(ValueError):
        ranking.pil_bilinear_tables(2048, 224)
    t = ranking.norm_table()
    assert t.shape == (3, 256) and t.dtype == np.float32
    assert t[1, 255] == (np.float32(255) / np.float32(255.0) - np.float32(0.456)) / np.float32(0.224)


@pytest.mark.parametrize("n", [1, 2, 3, 17, 50, 64])
def test_select_reference_is_rank_samples(n):
    for seed in range(4):
        disc, entr = score_lists(n, seed)
        best, disc_rank, entr_rank = ranking.select_reference(disc, entr)
        assert best == rank_samples(disc, entr)
        assert sorted(disc_rank) == sorted(entr_rank) == list(range(n))
        if n > 1:
            for which in range(2):          # one NaN in either list: it sorts after every number, in numpy's argsort too
                lists = [disc.copy(), entr.copy()]
                lists[which][seed % n] = np.nan
                best, *ranks = ranking.select_reference(*lists)
                assert best == rank_samples(*lists) and ranks[which][seed % n] == n - 1


def test_select_reference_puts_the_lower_index_first_among_equals():
    best, disc_rank, entr_rank = ranking.select_reference([1.0, 1.0, 0.0], [2.0, 2.0, 2.0])
    assert list(disc_rank) == [1, 2, 0] and list(entr_rank) == [0, 1, 2] and best == 0      # totals 3, 3, 0


def test_the_registry_has_the_rank_library():
    entry = next(e for e in _libraries.LIBRARIES if e.name == "rank")
    assert entry.so == "libpixelsynth_rank.so" and entry.headers == ("pixelsynth_rank.h",) and entry.last_error == "ps_rank_last_error"
    assert [u for u, _ in entry.units] == ["rank.hip"] and entry.units[0][1] == _libraries.NO_CONTRACT


def test_rank_library_exports_what_its_header_declares():
    protos = assert_library_matches_header("rank")
    assert set(protos) == set(_lib.RANK_PROTOS) == {"ps_rank_last_error", "ps_rank_classifier_input", "ps_rank_entropy",
                                                    "ps_rank_hinge_fake", "ps_rank_select"}
    assert _lib.call("ps_abi_version") == 2


def test_rank_entry_points_refuse_before_anything_is_launched():
    L = _lib.library("rank")
    assert L.ps_rank_classifier_input(None, 1, 256, 224, None, None, 5, None, None, None, None) != 0
    assert b"null pointer" in L.ps_rank_last_error()
    assert L.ps_rank_entropy(None, 1, 10, None, None) != 0 and b"null pointer" in L.ps_rank_last_error()
    assert L.ps_rank_hinge_fake(None, 1, None, 1, 1, None, None) != 0 and b"null pointer" in L.ps_rank_last_error()
    assert L.ps_rank_select(None, None, 2, None, None, None, None) != 0 and b"null pointer" in L.ps_rank_last_error()
    x = torch.zeros(4)
    p = x.data_ptr()                                   # (any non-null address: the shapes are refused before it is looked at)
    assert L.ps_rank_select(p, p, 2000, p, None, None, None) != 0 and b"n = 2000" in L.ps_rank_last_error()
    assert L.ps_rank_classifier_input(p, 1, 2048, 224, p, p, 5, p, p, None, None) != 0 and b"S = 2048" in L.ps_rank_last_error()
    assert L.ps_rank_entropy(p, 0, 10, p, None) != 0 and b"N = 0" in L.ps_rank_last_error()
    for fn, args in ((ranking.classifier_input, (torch.zeros(1, 3, 8, 8),)), (ranking.entropy, (torch.zeros(1, 4),)),
                     (ranking.hinge_fake, (torch.zeros(1, 1, 2, 2),) * 2), (ranking.select, (x, x))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(*args)


def test_rank_route_follows_the_argument_the_option_and_the_variable(monkeypatch):
    opt = argparse.Namespace()
    monkeypatch.delenv("PS_RANK", raising=False)
    assert _rank_route(None, opt) == "host" and _rank_route("device", opt) == "device"
    monkeypatch.setenv("PS_RANK", "device")
    assert _rank_route(None, opt) == "device" and _rank_route("host", opt) == "host"
    opt.rank_on = "host"
    assert _rank_route(None, opt) == "host" and _rank_route("device", opt) == "device"
    monkeypatch.setenv("PS_RANK", "gpu")
    opt.rank_on = None
    with pytest.raises(ValueError, match="PS_RANK is 'gpu'"):
        _rank_route(None, opt)
    with pytest.raises(ValueError, match="'bogus'"):
        _rank_route("bogus", opt)


def test_can_score_on_device_takes_the_mirror_in_hinge_mode_alone():
    from pixelsynth_amd.losses import DiscriminatorLoss
    from pixelsynth_amd.networks import resnet18
    opt = dict(discriminator_losses="pix2pixHD", norm_D="spectralinstance", ndf=8, output_nc=3, no_ganFeat_loss=False, isTrain=False,
               lambda_feat=10.0)
    hinge, ls = (DiscriminatorLoss(argparse.Namespace(gan_mode=g, **opt)) for g in ("hinge", "ls"))
    net = resnet18(num_classes=5)
    assert ranking.can_score_on_device(hinge, net) and not ranking.can_score_on_device(ls, net)

    class StandIn:
        def run_discriminator_one_step(self, fake, real):
            return {"D_Fake": fake.mean().reshape(1)}
    assert not ranking.can_score_on_device(StandIn(), net) and not ranking.can_score_on_device(hinge, None)
    assert not ranking.can_score_on_device(hinge, net, torch.zeros(1, 3, 16, 16))       # (a CPU tensor)
    with pytest.raises(RuntimeError, match="can_score_on_device"):
        ranking.score_candidates(torch.zeros(1, 3, 16, 16), hinge, net)
