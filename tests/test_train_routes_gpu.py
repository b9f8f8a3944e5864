"""GPU: the splits, chunks and walks of csrc/norm_train.hip, csrc/block_train.hip and csrc/conv_bwd.hip that the operator tests never take,
on the route cases of tests/_norm_train_ref.py, tests/_block_train_ref.py and tests/_conv_bwd_ref.py (tests/test_train_routes_cpu.py
asserts, without a GPU, that every case reaches its branch).  Everything goes through the C ABI.  The bounds are those of the reference
modules, unchanged but for the variance's m2 term (stat_bounds(x, rows=N), derived there for N > 2^12 rows); every check prints its
error / bound, and a test whose host reference is slow prints the time that took.  docs/LAB_NOTEBOOK.md has the table per case."""
import time

import pytest
import torch

import _block_train_ref as BR
import _conv_bwd_ref as CR
import _norm_train_ref as NR
from pixelsynth_amd import _lib
from pixelsynth_amd.networks import f16x3
from test_norm_train_gpu import EPS, _ops as norm_ops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CL = torch.channels_last
NAN = float("nan")
_REFS = {}
_WS = _lib.Workspace()


def _nhwc(t):
    return t.to(DEV).contiguous(memory_format=CL)


def _cached(key, make):
    """make() once per process -> (value, seconds it took the first time)"""
    if key not in _REFS:
        t0 = time.perf_counter()
        value = make()
        _REFS[key] = (value, time.perf_counter() - t0)
    return _REFS[key]


def _workspace(query, *sizes):
    """The workspace for these sizes, every byte 0xff: a slab element a kernel should have written and did not is a NaN in the sum"""
    ws = _WS.query(torch.device(DEV), query, *sizes)
    ws.fill_(255)
    return ws


# ---- the norm -------------------------------------------------------------------------------------------------------------------------------
def _norm_reference(shape, relu, shared):
    def make():
        B, C = shape[:2]
        x, gain, bias, dy = NR.inputs(*shape, seed=sum(shape), shared=shared)
        gain, bias = gain.expand(B, C).contiguous(), bias.expand(B, C).contiguous()          # (the entry points take (B, C) rows)
        f = NR.forward64(x, gain, bias, EPS, relu)
        flips = torch.zeros_like(dy, dtype=torch.bool)
        if relu:        # as tests/test_norm_train_gpu.py: no gradient through the values next to 0, where the mask may flip
            flips = f["v"].abs() < 1e-4
            assert flips.float().mean().item() <= 0.01
            dy = torch.where(flips, torch.zeros_like(dy), dy)
        g64 = NR.autograd(x, gain, bias, dy, EPS, relu, torch.float64)
        g32 = NR.autograd(x, gain, bias, dy, EPS, relu, torch.float32)
        return x, gain, bias, dy, f, g64, g32
    return _cached(("norm", shape, relu, shared), make)


_NORM = {c.id: c for c in NR.ROUTE_CASES}
NORM_RUNS = [(c.id, True, False) for c in NR.ROUTE_CASES if c.id != "single_value"] + [("chunk_tail", False, True)]


def _assert_a_nan_stays_in_its_channel(x, gain, bias, dy, clean, where):
    bad = x.clone()
    bad[where] = NAN
    ch = where[1]
    others = [c for c in range(x.size(1)) if c != ch]
    o = norm_ops(bad, gain, bias, dy=dy, relu=True)
    for k in ("mean", "var", "rstd", "stored_mean", "stored_var"):
        assert not torch.isfinite(o[k][ch]) and torch.equal(o[k][others], clean[k][others]), k
    for k in ("y", "dx", "dgain", "dbias"):
        assert not torch.isfinite(o[k][:, ch]).any() and torch.equal(o[k][:, others], clean[k][:, others]), k


@pytest.mark.parametrize("case,relu,shared", NORM_RUNS, ids=lambda v: v if isinstance(v, str) else None)
def test_norm_route_against_fp64(case, relu, shared):
    shape = _NORM[case].shape
    B, C, H, W = shape
    p = NR.plan(B, H * W, C)
    assert p.parts == _lib.call("ps_norm_train_parts", B, H * W, C)
    (x, gain, bias, dy, f, g64, g32), secs = _norm_reference(shape, relu, shared)
    name = f"{case} {'relu' if relu else 'linear'} {'shared' if shared else 'per-sample'}"
    gen = torch.Generator().manual_seed(1)
    stored = (torch.randn(C, generator=gen), torch.rand(C, generator=gen) + 0.5)
    pend = torch.randn(C, generator=gen)
    o = norm_ops(x, gain, bias, dy=dy, relu=relu, stored=stored, pend=pend)
    assert all(torch.isfinite(v).all() for v in o.values())
    mean_b, var_b = NR.stat_bounds(x, rows=B * H * W)
    assert NR.check(f"{name} mean", o["mean"], f["mean"], mean_b) <= 1.0
    assert NR.check(f"{name} var", o["var"], f["var"], var_b) <= 1.0
    assert torch.equal(o["rstd"].cpu(), (1.0 / torch.sqrt((o["var"].cpu() + EPS).double())).float())
    mean, var = o["mean"].cpu(), o["var"].cpu()
    assert torch.equal(o["stored_mean"].cpu(), stored[0] * 0.9 + (mean + pend) * 0.1)
    assert torch.equal(o["stored_var"].cpu(), stored[1] * 0.9 + var * 0.1)
    o2, o3 = norm_ops(x, gain, bias, relu=relu, stored=stored), norm_ops(x, gain, bias, relu=relu, stored=stored, keep=1.0, mom=1.0)
    assert torch.equal(o2["stored_mean"].cpu(), stored[0] * 0.9 + mean * 0.1) and torch.equal(o2["stored_var"].cpu(), stored[1] * 0.9 + var * 0.1)
    assert torch.equal(o3["stored_mean"].cpu(), stored[0] + mean) and torch.equal(o3["stored_var"].cpu(), stored[1] + var)
    assert all(torch.equal(o2[k], o[k]) and torch.equal(o3[k], o[k]) for k in ("mean", "var", "rstd", "y"))
    assert NR.check(f"{name} y", o["y"], f["y"], NR.forward_bound(x, f)) <= 1.0
    for what, w64, w32 in zip(("dx", "dgain", "dbias"), g64, g32):
        bound, E32 = NR.grad_bound(w32, w64)
        assert NR.check(f"{name} {what} (E32 / max |g64| {E32 / w64.abs().max().item():.2e})", o[what], w64, bound) <= 1.0, what
    again = norm_ops(x, gain, bias, dy=dy, relu=relu, stored=stored, pend=pend)
    assert all(torch.equal(o[k], again[k]) for k in o)
    if relu and case == "chunk_tail":            # the last channel of the last chunk, a row of the last lane
        _assert_a_nan_stays_in_its_channel(x, gain, bias, dy, norm_ops(x, gain, bias, dy=dy), (0, C - 1, H - 1, W - 1))
    if case == "many_parts_per_frame":          # the last part of frame 1 (its one row past the 64 full parts)
        assert (H - 1) * W >= (p.ppf - 1) * p.part_rows
        _assert_a_nan_stays_in_its_channel(x, gain, bias, dy, norm_ops(x, gain, bias, dy=dy), (1, C - 1, H - 1, 7))
    print(f"{name}: host reference {secs:.2f} s")


def test_norm_of_a_single_value():
    """n = 1: the mean is x and the variance an exact 0 (x^2 and mean^2 are the same fp64 number), so rstd is 1 / sqrt(eps) and
    v = bias; dx is the difference of gain * g, rounded once on each side, and an xhat of 0: within 4 u |rstd gain dy|"""
    shape = _NORM["single_value"].shape
    (x, gain, bias, dy, f, g64, g32), _ = _norm_reference(shape, True, False)
    gen = torch.Generator().manual_seed(1)
    stored, pend = (torch.randn(4, generator=gen), torch.rand(4, generator=gen) + 0.5), torch.randn(4, generator=gen)
    o = norm_ops(x, gain, bias, dy=dy, relu=True, stored=stored, pend=pend)
    assert torch.equal(o["mean"].cpu(), x.flatten()) and not o["var"].any()
    assert torch.equal(o["stored_mean"].cpu(), stored[0] * 0.9 + (x.flatten() + pend) * 0.1) and torch.equal(o["stored_var"].cpu(), stored[1] * 0.9)
    eps32 = torch.tensor(EPS, dtype=torch.float32)
    assert torch.equal(o["rstd"].cpu(), (1.0 / torch.sqrt(eps32.double())).float().expand(4))
    assert NR.check("single value y", o["y"], f["y"], NR.forward_bound(x, f)) <= 1.0
    for what, w64, w32 in zip(("dgain", "dbias"), g64[1:], g32[1:]):
        bound, _ = NR.grad_bound(w32, w64)
        assert NR.check(f"single value {what}", o[what], w64, bound) <= 1.0
    dx = o["dx"].cpu().double()
    limit = 4 * NR.U * (o["rstd"].cpu().double().view(1, 4, 1, 1) * gain.double().view(1, 4, 1, 1) * dy.double()).abs()
    print(f"single value dx: max |dx| {dx.abs().max().item():.3e}, largest limit {limit.max().item():.3e}")
    assert torch.isfinite(dx).all() and (dx.abs() <= limit).all()
    again = norm_ops(x, gain, bias, dy=dy, relu=True, stored=stored, pend=pend)
    assert all(torch.equal(o[k], again[k]) for k in o)


# ---- the 1 x 1 convolution's weight and bias gradient ---------------------------------------------------------------------------------------------
from _rims import GUARD, SENTINEL, guarded as _guarded, untouched as _untouched  # noqa: E402,F401  (the route tests take them from here)


def _gw_reference(shape):
    def make():
        x, w, b, g = BR.gw_inputs(*shape)
        return x, w, b, g, BR.conv1x1_grads(x, w, b, g), BR.conv1x1_grads(x, w, b, g, torch.float32)
    return _cached(("gw",) + shape, make)


@pytest.mark.parametrize("shape", BR.GW_ROUTE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_grad_weight_route_against_fp64(shape):
    npix, Ci, Co = shape
    p = BR.gw_plan(*shape)
    assert p.parts == _lib.call("ps_conv1x1_grad_weight_parts", *shape)
    (x, w, b, g, g64, g32), secs = _gw_reference(shape)
    xd, gd = _nhwc(x), _nhwc(g)
    wbuf, gw = _guarded(Co * Ci)
    bbuf, gb = _guarded(Co)
    ws = _workspace("ps_conv1x1_grad_weight_workspace_bytes", *shape)
    _lib.call("ps_conv1x1_grad_weight_f32", xd, gd, npix, Ci, Co, gw, gb, ws, ws.numel())
    torch.cuda.synchronize()
    assert torch.isfinite(gw).all() and torch.isfinite(gb).all()                        # every element was written ...
    assert _untouched(wbuf, Co * Ci) and _untouched(bbuf, Co)                           # ... and none outside (Co, Ci) and (Co)
    gw = gw.view(Co, Ci, 1, 1)
    name = f"{shape} <{p.TO},{p.TC}> {p.tiles_o} x {p.tiles_c} tiles, {p.parts} parts of {p.part_pix}"
    for what, got, want, w32 in (("grad_weight", gw, g64[1], g32[1]), ("grad_bias", gb, g64[2], g32[2])):
        bound, E32 = BR.grad_bound(w32, want)
        assert BR.check(f"{name} {what}, the project's rule (E32 {E32:.3e}, max |g64| {want.abs().max().item():.3e})", got, want, bound) <= 1.0
    L = BR.chain(*shape)
    assert BR.check(f"{name} grad_weight, (L + parts) u sum |g||x| (L = {L})", gw, g64[1], BR.grad_weight_bound(x, g, *shape)) <= 1.0
    # without the bias: the same weight gradient, nothing written to a bias
    wbuf2, gw2 = _guarded(Co * Ci)
    ws = _workspace("ps_conv1x1_grad_weight_workspace_bytes", *shape)
    _lib.call("ps_conv1x1_grad_weight_f32", xd, gd, npix, Ci, Co, gw2, None, ws, ws.numel())
    torch.cuda.synchronize()
    assert torch.equal(gw2, gw.flatten()) and _untouched(wbuf2, Co * Ci)
    print(f"{name}: host reference {secs:.2f} s")


# ---- the resampling adjoints -----------------------------------------------------------------------------------------------------------------------
def _adjoint_abi(kind, gd, shape4):
    B, H, W, C = shape4
    gin = torch.full((B, C, H, W), NAN, device=DEV).contiguous(memory_format=CL)
    _lib.call("ps_upsample_add_bwd_nhwc_f32" if kind == "Up" else "ps_pool_add_bwd_nhwc_f32", gd, B, H, W, C, gin)
    torch.cuda.synchronize()
    return gin


def _adjoint_reference(kind, shape4):
    def make():
        B, H, W, C = shape4
        shape = (B, C, H, W)
        gen = torch.Generator().manual_seed(sum(shape4))
        Ho, Wo = (2 * H, 2 * W) if kind == "Up" else (H // 2, W // 2)
        g = torch.randn(B, C, Ho, Wo, generator=gen)
        return shape, g, BR.adjoint(kind, g, shape), BR.adjoint_bound(kind, g, shape)
    return _cached(("adjoint", kind) + shape4, make)


@pytest.mark.parametrize("kind,shape4", [("Up", s) for s in BR.UP_ROUTE_SHAPES] + [("Down", s) for s in BR.DOWN_ROUTE_SHAPES],
                         ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_adjoint_route_against_fp64(kind, shape4):
    (shape, g, y64, bound), secs = _adjoint_reference(kind, shape4)
    B, H, W, C = shape4
    total4, rest, rows = BR.second_trip(shape4)
    got = _adjoint_abi(kind, _nhwc(g), shape4)
    assert got.shape == shape and got.is_contiguous(memory_format=CL)
    assert BR.check(f"{kind} {shape4} adjoint, k u sum |w g|", got, y64, bound) <= 1.0
    if rest:           # what a thread computes on its second trip of the grid-stride loop: the last rows of the last frame, border included
        assert rows == 4
        tail = (slice(B - 1, B), slice(None), slice(H - rows, H))
        assert BR.check(f"{kind} {shape4} adjoint, the second trip's {rows} rows", got[tail], y64[tail], bound[tail]) <= 1.0
        assert got[tail].abs().max() > 0.1
        assert torch.equal(got, _adjoint_abi(kind, _nhwc(g), shape4))
    else:
        assert W == 1 and kind == "Up" and (BR.adjoint_terms(kind, shape) == torch.tensor([6.0, 8.0, 6.0]).view(1, 1, 3, 1)).all()
    print(f"{kind} {shape4}: host reference {secs:.2f} s")


# ---- the 3 x 3 convolution's backward pass ---------------------------------------------------------------------------------------------------
def _conv_abi(x, w, g):
    """One backward pass through the entry points, as networks/f16x3.py chains them -> (grad_x, grad_w (Co, Ci, 3, 3), grad_bias,
    scale2 on the host, the grad_weight kernel's overflow word, the word of the forward kernel that ran on the gradient)"""
    B, Ci, H, W = x.shape
    Co = w.size(0)
    xd, gd = _nhwc(x), _nhwc(g)
    gs = torch.full_like(gd, NAN)
    assert gs.is_contiguous(memory_format=CL)
    scale2, gb = torch.full((2,), NAN, device=DEV), torch.full((Co,), NAN, device=DEV)
    ws = _workspace("ps_conv3x3_bwd_workspace_bytes", B, H, W, Ci, Co)
    _lib.call("ps_conv3x3_bwd_prepare_f32", gd, B, H, W, Co, gs, scale2, gb, ws, ws.numel())
    ws.fill_(255)
    over, gover = torch.zeros(1, dtype=torch.int32, device=DEV), torch.zeros(1, dtype=torch.int32, device=DEV)
    gw = torch.full((Co, 3, 3, Ci), NAN, device=DEV)
    _lib.call("ps_conv3x3_grad_weight_f16x3", xd, gs, scale2, B, H, W, Ci, Co, gw, over, ws, ws.numel())
    gx = f16x3.conv3x3(gs, f16x3.pack3x3(w.to(DEV).flip(2, 3).transpose(0, 1), check=False), overflow=gover)
    _lib.call("ps_conv3x3_bwd_unscale_f32", gx, gx.numel(), scale2)
    torch.cuda.synchronize()
    return gx, gw.permute(0, 3, 1, 2), gb, scale2.cpu(), int(over.item()), int(gover.item())


def _conv_reference(shape):
    """The case's inputs and Reference: once per process (the largest case's is some 5 GMAC per fp64 pass on the host)"""
    def make():
        x, w, b, g = CR.inputs(*shape)
        return x, w, b, g, CR.reference(x, w, g)
    return _cached(("conv",) + shape, make)


@pytest.mark.parametrize("case", CR.ROUTE_CASES, ids=lambda c: c.id)
def test_conv_bwd_route_against_fp64(case):
    """_conv_bwd_ref.check's two assertions, unchanged.  Neither counts summands: the first compares with torch's fp32 evaluation of the
    same products at the same sizes, the second with torch's fp32 backward at the same sizes -- both grow with the reduction as the
    kernel's own error does."""
    shape = case.shape
    p = CR.plan(*shape)
    assert p.parts == _lib.call("ps_conv3x3_bwd_parts", *shape)
    (x, w, b, g, r), secs = _conv_reference(shape)
    t0 = time.perf_counter()
    gx, gw, gb, scale2, over, gover = _conv_abi(x, w, g)
    dev_secs = time.perf_counter() - t0
    s = CR.scale_of(g.abs().max().item())
    assert scale2.tolist() == [s, 1.0 / s] and r.s == s and over == 0 and gover == 0
    name = f"{case.id} {'x'.join(map(str, shape))} ({p.parts} parts of {p.chunk} tiles, {p.nprep} ranges of {p.pchunk} pixels)"
    assert gx.shape == x.shape and gx.is_contiguous(memory_format=CL) and gw.shape == w.shape and gb.shape == b.shape
    CR.check(f"{name} grad_input", gx, r.x)
    CR.check(f"{name} grad_weight", gw, r.weight)
    CR.check(f"{name} grad_bias", gb, r.bias)
    print(f"{name}: host reference {secs:.2f} s, device pass with copies {dev_secs:.2f} s")
