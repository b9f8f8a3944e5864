"""CPU-only: the one resolver behind get_best_sample's rank_on and rank_scope (best_sample.resolve_option): the argument over the option
over the environment variable over the default, a default of None for "nothing was asked for", and the texts of its refusals."""
import argparse

import pytest

from pixelsynth_amd.best_sample import RANK_ROUTES, RANK_SCOPES, resolve_option


def route(arg, opt, default="host"):
    return resolve_option(arg, opt, "rank_on", "PS_RANK", RANK_ROUTES, default)


def test_argument_over_option_over_variable_over_default(monkeypatch):
    opt = argparse.Namespace()
    monkeypatch.delenv("PS_RANK", raising=False)
    assert route(None, opt) == "host" and route(None, None) == "host"               # nothing set: the default
    monkeypatch.setenv("PS_RANK", "device")
    assert route(None, opt) == "device"                                              # the variable over the default
    opt.rank_on = "host"
    assert route(None, opt) == "host"                                                # the option over the variable
    assert route("device", opt) == "device"                                          # the argument over the option
    opt.rank_on = None                                                               # (an option left at None is not set)
    assert route(None, opt) == "device" and route("host", opt) == "host"


def test_the_variable_is_read_at_every_call(monkeypatch):
    opt = argparse.Namespace()
    monkeypatch.setenv("PS_RANK_SCOPE", "view")
    assert resolve_option(None, opt, "rank_scope", "PS_RANK_SCOPE", RANK_SCOPES, "batch") == "view"
    monkeypatch.setenv("PS_RANK_SCOPE", "batch")
    assert resolve_option(None, opt, "rank_scope", "PS_RANK_SCOPE", RANK_SCOPES, "batch") == "batch"
    monkeypatch.delenv("PS_RANK_SCOPE")
    assert resolve_option(None, opt, "rank_scope", "PS_RANK_SCOPE", RANK_SCOPES, "batch") == "batch"


def test_a_default_of_none_says_that_nothing_was_asked_for(monkeypatch):
    opt = argparse.Namespace(rank_on=None)
    monkeypatch.delenv("PS_RANK", raising=False)
    assert route(None, opt, default=None) is None
    monkeypatch.setenv("PS_RANK", "host")
    assert route(None, opt, default=None) == "host"
    opt.rank_on = "device"
    assert route(None, opt, default=None) == "device" and route("host", opt, default=None) == "host"


def test_refusals_name_the_three_places_and_the_value(monkeypatch):
    opt = argparse.Namespace()
    monkeypatch.setenv("PS_RANK", "gpu")
    with pytest.raises(ValueError, match=r"get_best_sample: rank_on / opt\.rank_on / PS_RANK is 'gpu', expected one of \('host', 'device'\)"):
        route(None, opt)
    with pytest.raises(ValueError, match="PS_RANK is 'gpu'"):
        route(None, opt, default=None)                                               # (the default does not excuse a misspelt value)
    assert route("host", opt) == "host"                                              # a valid argument is not held up by the variable
    monkeypatch.setenv("PS_RANK_SCOPE", "scene")
    with pytest.raises(ValueError, match=r"get_best_sample: rank_scope / opt\.rank_scope / PS_RANK_SCOPE is 'scene', expected one of "
                                         r"\('batch', 'view'\)"):
        resolve_option(None, opt, "rank_scope", "PS_RANK_SCOPE", RANK_SCOPES, "batch")
    for empty in ("", "Host"):
        monkeypatch.setenv("PS_RANK", empty)
        with pytest.raises(ValueError, match=f"PS_RANK is {empty!r}"):
            route(None, opt)
