"""tools/_measure.py on the device, around one launch of the smallest kernel the library has (k_add_bias on 64 floats): the event timer,
the profiler's device events and their reduction, a round of alternation, the looped timer.  No time is asserted beyond its sign."""
import math
import os
import sys

import pytest
import torch

from pixelsynth_amd import _lib

TOOLS = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
if TOOLS not in sys.path:
    sys.path.append(TOOLS)

import _measure  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def launch():
    cl = torch.channels_last
    a, b = (torch.randn(1, 4, 4, 4, device="cuda:0").contiguous(memory_format=cl) for _ in range(2))
    bias, out = torch.randn(4, device="cuda:0"), torch.empty(1, 4, 4, 4, device="cuda:0").contiguous(memory_format=cl)
    return lambda: _lib.call("ps_add_bias_nhwc_f32", a, b, bias, 1, 16, 4, out)


def test_event_ms(launch):
    ms = _measure.event_ms(launch)
    assert isinstance(ms, float) and math.isfinite(ms) and ms > 0


def test_device_events_and_medians(launch):
    events = _measure.device_events(launch, 3)
    mine = [ms for name, ms in events if "k_add_bias" in name]
    assert len(mine) == 3 and all(ms > 0 for ms in mine), events
    assert list(_measure.kernel_medians(events, ("k_add_bias",))) == ["k_add_bias"]


def test_alternate(launch):
    med = _measure.alternate({"x": launch, "y": launch}, rounds=2, calls=2)
    assert sorted(med) == ["x", "y"]
    assert all(len(v) == 2 and all(m > 0 for m in v) for v in med.values()), med


def test_looped_ms(launch):
    assert _measure.looped_ms(launch, 4, 1) > 0
