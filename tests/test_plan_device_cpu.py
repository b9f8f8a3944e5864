"""CPU-only: the C ABI of libpixelsynth_plan.so (the AR plan's orders on the device, csrc/ar_order.hip) against its header and bindings,
its shape query, and what build_ar_plan's order_on switch refuses before it touches a device."""
import pytest
import torch

from abi_util import assert_library_matches_header
from pixelsynth_amd import _lib, _libraries
from pixelsynth_amd.ar_plan import build_ar_plan


def test_the_registry_has_the_plan_library():
    entry = next(e for e in _libraries.LIBRARIES if e.name == "plan")
    assert entry.so == "libpixelsynth_plan.so" and entry.headers == ("pixelsynth_plan.h",) and entry.last_error == "ps_plan_last_error"
    assert [u for u, _ in entry.units] == ["ar_order.hip"]


def test_plan_library_exports_what_its_header_declares():
    """include/pixelsynth_plan.h, the exports of libpixelsynth_plan.so and _lib.PLAN_PROTOS name the same three entry points with the
    same number of parameters; libpixelsynth_hip.so's ABI version stays 2 (its 69 prototypes: tests/test_abi.py)."""
    protos = assert_library_matches_header("plan")
    assert set(protos) == set(_lib.PLAN_PROTOS) == {"ps_plan_last_error", "ps_plan_order_takes", "ps_plan_order"}
    assert _lib.call("ps_abi_version") == 2


@pytest.mark.parametrize("S,G,takes", [(256, 32, 1), (32, 32, 1), (24, 8, 1), (4, 4, 1), (256, 64, 0), (100, 32, 0), (0, 32, 0)])
def test_plan_order_takes(S, G, takes):
    assert _lib.call("ps_plan_order_takes", S, G) == takes


def test_plan_order_refuses_host_tensors_before_touching_a_stream():
    bg = torch.ones(1, 32, 32, dtype=torch.uint8)
    order, region = torch.zeros(1, 1024, dtype=torch.int32), torch.zeros(1, 1024, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match=r"ps_plan_order: args\[0\] is a CPU tensor.*no CPU fallback"):
        _lib.call("ps_plan_order", bg, 1, 32, 32, order, region, None, None)
    # and the library itself, before anything is launched: NULL pointers, a refused shape
    L = _lib.library("plan")
    assert L.ps_plan_order(None, 1, 32, 32, None, None, None, None, None) != 0 and b"null pointer" in L.ps_plan_last_error()


def test_build_ar_plan_device_route_refuses_a_host_mask():
    with pytest.raises(ValueError, match="on the device"):
        build_ar_plan(torch.ones(1, 256, 256, dtype=torch.bool), order_on="device")


def test_build_ar_plan_refuses_an_unknown_route(monkeypatch):
    mask = torch.ones(1, 256, 256, dtype=torch.bool)
    with pytest.raises(ValueError, match="bogus"):
        build_ar_plan(mask, order_on="bogus")
    monkeypatch.setenv("PS_PLAN_ORDER", "gpu")
    with pytest.raises(ValueError, match="PS_PLAN_ORDER.*'gpu'"):
        build_ar_plan(mask)
    monkeypatch.setenv("PS_PLAN_ORDER", "device")       # the variable reaches the default: the device route refuses the host mask
    with pytest.raises(ValueError, match="on the device"):
        build_ar_plan(mask)
