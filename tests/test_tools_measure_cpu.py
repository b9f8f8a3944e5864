"""tools/_measure.py, the measuring protocol behind the *_time.py tools, without a device: the order in which alternate() times its
routes and what it keeps of the times, span, the ownership rule of kernel_medians, that every converted tool's parser loads, and that
_measure pulls in nothing of pixelsynth_amd.  No time is asserted."""
import importlib
import os
import subprocess
import sys

import pytest

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.append(TOOLS)

import _measure  # noqa: E402

CONVERTED = ("block_train_time", "content_loss_time", "conv_bwd_time", "lmconv_bwd_time", "nll_time", "norm_train_time", "thin_train_time",
             "vq_train_time", "splat_bwd_time", "gan_train_time", "pixelcnn_train_time", "consistency_time", "metrics_time", "fid_time",
             "scene_time")


def _never():
    raise AssertionError("alternate() called a route outside event_ms")


def _scripted(monkeypatch, times):
    """event_ms replaced: notes which route it was given and hands back the next of `times`; the routes themselves never run"""
    a, b = (lambda: _never()), (lambda: _never())
    names, left, order = {a: "a", b: "b"}, list(times), []

    def recorder(fn):
        order.append(names[fn])
        return left.pop(0)
    monkeypatch.setattr(_measure, "event_ms", recorder)
    return {"a": a, "b": b}, order, left


WARM6 = [100.0, 200.0, 300.0, 400.0, 500.0, 600.0]
#         a     b     a     b   | a    b    a    b
ROUNDS = [1.0, 10.0, 3.0, 30.0, 5.0, 7.0, 2.0, 8.0]


def test_alternate_call_order(monkeypatch):
    routes, order, left = _scripted(monkeypatch, WARM6 + ROUNDS)
    _measure.alternate(routes, rounds=2, calls=2, warm=3)
    assert order == list("ababab") + list("abab") + list("abab")
    assert left == []


def test_alternate_result(monkeypatch):
    routes, _, _ = _scripted(monkeypatch, WARM6 + ROUNDS)
    assert _measure.alternate(routes, rounds=2, calls=2) == {"a": [2.0, 3.5], "b": [20.0, 7.5]}      # (warm=3 is the default)
    # warm=2: four calls are dropped, so the same script's last two warm-up times become the first round's first pair
    routes, order, left = _scripted(monkeypatch, WARM6 + ROUNDS[:6])
    assert _measure.alternate(routes, rounds=2, calls=2, warm=2) == {"a": [250.5, 4.0], "b": [305.0, 18.5]}
    assert order == list("abab") + list("abab") + list("abab") and left == []


def test_span():
    assert _measure.span([0.123456, 2.000049, 1.0]) == [0.1235, 2.0]
    assert _measure.span([3.14159]) == [3.1416, 3.1416]


def test_kernel_medians():
    events = [("void ns::k_stats_finish<4>(Args)", 1.0), ("k_stats(Args)", 2.0), ("k_stats(Args)", 4.0), ("Cijk_something", 9.0),
              ("k_apply", 0.33333), ("k_apply", 0.5), ("k_apply", 0.7), ("k_apply", 100.0)]
    assert _measure.kernel_medians(events, ("k_stats_finish", "k_stats", "k_apply")) == {"k_stats_finish": 1.0, "k_stats": 3.0, "k_apply": 0.6}
    # the shorter name first takes the longer name's event too
    assert _measure.kernel_medians(events, ("k_stats", "k_stats_finish", "k_apply")) == {"k_stats": 2.0, "k_apply": 0.6}
    assert _measure.kernel_medians(events[4:6], ("k_apply",)) == {"k_apply": 0.4167}                 # rounded to 4 places
    assert _measure.kernel_medians([], ("k_stats",)) == {}
    assert _measure.kernel_medians(events, ()) == {}


@pytest.mark.parametrize("tool", CONVERTED)
def test_parser_loads_without_a_device(tool, capsys):
    path = list(sys.path)
    try:
        module = importlib.import_module(tool)
        with pytest.raises(SystemExit) as stop:
            module.main(["--help"])
    finally:
        sys.path[:] = path
    assert stop.value.code == 0
    assert "usage:" in capsys.readouterr().out


def test_measure_imports_nothing_of_the_package():
    code = ("import sys; sys.path.insert(0, %r); import _measure; "
            "mine = sorted(m for m in sys.modules if m.split('.')[0] == 'pixelsynth_amd'); assert not mine, mine" % TOOLS)
    done = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert done.returncode == 0, done.stderr
