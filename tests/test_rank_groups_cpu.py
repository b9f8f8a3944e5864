"""CPU-only: the host side of best-of-N per view (get_best_sample's rank_scope="view"): the numpy restatement of the per-group rank rule
against select_reference, the draws every view of a batch gets, what decides the scope, the C ABI of libpixelsynth_rank_groups.so against
its header and bindings, and the driver's argument errors."""
import argparse

import numpy as np
import pytest
import torch

from abi_util import assert_library_matches_header
from pixelsynth_amd import _lib, _libraries, driver, ranking
from pixelsynth_amd.z_buffermodel import _rank_scope, view_draws
from rank_util import select_cases


def lay_out(per_group, layout):
    """[(disc, entr) of n scores each] -> the two flat lists in `layout`"""
    groups, n = len(per_group), len(per_group[0][0])
    gs, cs = ranking.group_strides(groups, n, layout)
    flat = np.empty((2, groups * n), np.float32)
    for g, lists in enumerate(per_group):
        flat[:, g * gs + np.arange(n) * cs] = lists
    return flat[0], flat[1]


@pytest.mark.parametrize("layout", ranking.LAYOUTS)
@pytest.mark.parametrize("n", [1, 2, 17, 50, 64])
def test_select_groups_reference_is_select_reference_group_by_group(n, layout):
    per_group = [c for c in select_cases() if len(c[0]) == n]
    per_group += [(np.full(n, 0.25, np.float32), np.full(n, 2.0, np.float32))]          # all equal: the lowest index
    groups = len(per_group)
    assert groups >= 3
    gs, cs = ranking.group_strides(groups, n, layout)
    assert (gs, cs) == ((1, groups) if layout == "candidate_major" else (n, 1))
    disc, entr = lay_out(per_group, layout)
    best, disc_rank, entr_rank = ranking.select_groups_reference(disc, entr, groups, n, layout)
    assert best.shape == (groups,) and disc_rank.shape == entr_rank.shape == (groups * n,)
    for g, (d, e) in enumerate(per_group):
        want, want_d, want_e = ranking.select_reference(d, e)
        at = g * gs + np.arange(n) * cs
        assert best[g] == want and np.array_equal(disc_rank[at], want_d) and np.array_equal(entr_rank[at], want_e), g
    assert best[-1] == 0
    if n > 1:
        with pytest.raises(ValueError, match="expected two lists"):
            ranking.select_groups_reference(disc[1:], entr, groups, n, layout)
    with pytest.raises(ValueError, match="'row_major'"):
        ranking.group_strides(groups, n, "row_major")


def test_view_draws_are_the_b1_draws_of_every_candidate():
    n, B, L = 3, 4, 1024
    draws = view_draws(n, B, L)
    assert tuple(draws.shape) == (n, B, L) and draws.dtype == torch.float32
    for i in range(n):
        want = torch.rand(1, L, generator=torch.Generator(device="cpu").manual_seed(i))     # what a B = 1 run of get_best_sample draws
        for b in range(B):
            assert torch.equal(draws[i, b], want[0]), (i, b)
    rows = torch.rand(B, L, generator=torch.Generator(device="cpu").manual_seed(1))
    assert not torch.equal(draws[1, 1], rows[1])                                             # (never row b of a (B, L) draw)
    assert not torch.equal(draws[0], draws[1])


def test_rank_scope_follows_the_argument_the_option_and_the_variable(monkeypatch):
    opt = argparse.Namespace()
    monkeypatch.delenv("PS_RANK_SCOPE", raising=False)
    assert _rank_scope(None, opt) == "batch" and _rank_scope("view", opt) == "view"
    monkeypatch.setenv("PS_RANK_SCOPE", "view")
    assert _rank_scope(None, opt) == "view" and _rank_scope("batch", opt) == "batch"
    opt.rank_scope = "batch"
    assert _rank_scope(None, opt) == "batch" and _rank_scope("view", opt) == "view"
    monkeypatch.setenv("PS_RANK_SCOPE", "scene")
    opt.rank_scope = None
    with pytest.raises(ValueError, match="PS_RANK_SCOPE is 'scene'"):
        _rank_scope(None, opt)
    with pytest.raises(ValueError, match="'frame'"):
        _rank_scope("frame", opt)


def test_the_registry_has_the_rank_groups_library():
    entry = next(e for e in _libraries.LIBRARIES if e.name == "rank_groups")
    assert entry.so == "libpixelsynth_rank_groups.so" and entry.headers == ("pixelsynth_rank_groups.h",)
    assert entry.last_error == "ps_rank_groups_last_error"
    assert [u for u, _ in entry.units] == ["rank_groups.hip"] and entry.units[0][1] == _libraries.NO_CONTRACT
    protos = assert_library_matches_header("rank_groups")
    assert set(protos) == set(_lib.RANK_GROUPS_PROTOS) == {"ps_rank_groups_last_error", "ps_rank_select_groups", "ps_rank_take_groups"}
    assert ranking.MAX_GROUPS == 65535 and ranking.SCORE_CHUNK == 64


def test_rank_groups_entry_points_refuse_before_anything_is_launched():
    L = _lib.library("rank_groups")
    err = L.ps_rank_groups_last_error
    assert L.ps_rank_select_groups(None, None, 2, 2, 1, 2, None, None, None, None) != 0 and b"null pointer" in err()
    assert L.ps_rank_take_groups(None, None, 2, 2, 1, 2, 4, None, None) != 0 and b"null pointer" in err()
    x = torch.zeros(4)
    p = x.data_ptr()                                   # (any non-null address: the shapes are refused before it is looked at)
    assert L.ps_rank_select_groups(p, p, 2, 0, 1, 2, p, None, None, None) != 0 and b"n = 0" in err()
    assert L.ps_rank_select_groups(p, p, 2, 1025, 1, 2, p, None, None, None) != 0 and b"n = 1025" in err()
    assert L.ps_rank_select_groups(p, p, 65536, 2, 1, 65536, p, None, None, None) != 0 and b"groups = 65536" in err()
    assert L.ps_rank_select_groups(p, p, 0, 2, 1, 0, p, None, None, None) != 0 and b"groups = 0" in err()
    assert L.ps_rank_select_groups(p, p, 3, 2, 2, 3, p, None, None, None) != 0 and b"strides (group 2, candidate 3)" in err()
    assert L.ps_rank_take_groups(p, p, 3, 2, 1, 2, 4, p, None) != 0 and b"strides (group 1, candidate 2)" in err()
    assert L.ps_rank_take_groups(p, p, 3, 2, 1, 3, 0, p, None) != 0 and b"item_floats = 0" in err()
    assert L.ps_rank_take_groups(p, p, 65536, 2, 2, 1, 4, p, None) != 0 and b"groups = 65536" in err()
    for fn, args in ((ranking.select_groups, (x, x, 2, 2)), (ranking.take_groups, (x, torch.zeros(2, dtype=torch.int32), 2))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            fn(*args)


def test_score_candidates_refuses_a_chunk_below_one():
    with pytest.raises(ValueError, match="chunk = 0"):
        ranking.score_candidates(torch.zeros(1, 3, 16, 16), None, None, 0)


def test_driver_argument_errors_come_before_any_device_is_touched(monkeypatch, tmp_path, capsys):
    def touched(*a, **kw):
        raise AssertionError("the driver touched the device before it refused its arguments")
    monkeypatch.setattr(torch.cuda, "set_device", touched)
    monkeypatch.setattr(driver, "build_model", touched)
    monkeypatch.setattr(driver, "build_scorers", touched)
    some = str(tmp_path / "weights.pt")
    for argv, said in ((["--scene", "R", "--num-samples", "2"], "--discriminator PATH and --classifier PATH"),
                       (["--scene", "R", "--num-samples", "2", "--discriminator", some], "--discriminator PATH and --classifier PATH"),
                       (["--scene", "R", "--num-samples", "2", "--classifier", some], "--discriminator PATH and --classifier PATH"),
                       (["--scene", "R", "--num-samples", "0"], "--num-samples must be >= 1")):
        with pytest.raises(SystemExit) as exit_:
            driver.main(argv + ["--out", str(tmp_path / "out")])
        assert exit_.value.code == 2 and said in capsys.readouterr().err, argv
    assert not (tmp_path / "out").exists()
