"""GPU: the chunks, walks, tiles and steps of csrc/splat_bwd.hip, csrc/vq_train.hip and csrc/lmconv_bwd.hip that the operator tests never
take, on the route cases of tests/_splat_bwd_ref.py, tests/_vq_train_ref.py and tests/_lmconv_bwd_ref.py (tests/test_train_routes2_cpu.py
asserts, without a GPU, that every case reaches its branch).  Each case goes through the module as the operator tests do -- their own
helpers, their bars and derived bounds unchanged -- and then through the C ABI with every output NaN-filled inside sentinel rims and the
workspace's every byte 0xff: an element left unwritten, a store outside an output and a slab read before it was written all show.  Every
check prints its error / bound; docs/LAB_NOTEBOOK.md section 14 has the table per case."""
import numpy as np
import pytest
import torch

import _lmconv_bwd_ref as LR
import _splat_bwd_ref as SR
import _vq_train_ref as VR
import test_splat_bwd_gpu as splat_ops
import test_vq_train_gpu as vq_ops
from pixelsynth_amd import _lib
from test_lmconv_bwd_gpu import _check_case, _hip_gradients
from test_train_routes_gpu import GUARD, _guarded, _untouched, _workspace

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INT_SENTINEL, INT_FILL, POISON = -12345, -777, 1000.0


def _guarded_int(n):
    buf = torch.full((GUARD + n + GUARD,), INT_SENTINEL, dtype=torch.int32, device=DEV)
    buf[GUARD:GUARD + n] = INT_FILL
    return buf, buf[GUARD:GUARD + n]


def _untouched_int(buf, n):
    return bool((buf[:GUARD] == INT_SENTINEL).all() and (buf[GUARD + n:] == INT_SENTINEL).all())


# ---- the splat's backward pass ---------------------------------------------------------------------------------------------------------------
def _splat_abi(c, neg, feat, idx, dist, g, want_pts=True, want_feat=True):
    """ps_splat_backward_f32 on the debug route's lists -> (grad_pts (B,N,3) or None, grad_feat (B,C,N) or None), each asserted written
    everywhere and nowhere else"""
    from pixelsynth_amd.layers.z_buffer_layers import ACCUMULATION
    npts, nfeat = c.B * c.N * 3, c.B * c.C * c.N
    pbuf, gp = _guarded(npts) if want_pts else (None, None)
    fbuf, gf = _guarded(nfeat) if want_feat else (None, None)
    ws = _workspace("ps_splat_bwd_workspace_bytes", c.B, c.S, c.K)
    _lib.call("ps_splat_backward_f32", neg, feat, idx, dist, g, c.B, c.N, c.C, c.S, float(c.r), c.K, float(c.tau), c.rad_pow,
              ACCUMULATION[c.acc], gp, gf, ws, ws.numel())
    torch.cuda.synchronize()
    if want_pts:
        assert torch.isfinite(gp).all() and _untouched(pbuf, npts)
    if want_feat:
        assert torch.isfinite(gf).all() and _untouched(fbuf, nfeat)
    return gp.view(c.B, c.N, 3) if want_pts else None, gf.view(c.B, c.C, c.N) if want_feat else None


@pytest.mark.parametrize("case", SR.ROUTE_CASES, ids=lambda c: c.id)
def test_splat_bwd_route_against_fp64(case):
    c = case
    gp, gf, idx, dist = splat_ops.check_gradients(c)          # through the module: the operator test's body, its bar unchanged
    pts, feat, o, g = splat_ops._reference(c)[:4]
    neg = torch.tensor(pts, device=DEV)
    neg[..., :2] = -neg[..., :2]                               # what the forward saved: the caller's points with x and y negated
    assert np.array_equal(neg.cpu().numpy(), o["pts_after"])
    dfeat, dg = torch.tensor(feat, device=DEV), torch.tensor(g, device=DEV)
    gp2, gf2 = _splat_abi(c, neg, dfeat, idx, dist, dg)
    assert torch.equal(gp2, gp) and torch.equal(gf2, gf)
    assert gf.abs().amax((0, 2)).min() > 0, "a channel without a gradient: a lane or a chunk that proves nothing"
    if c.id in ("bwd_C70_tau2", "bwd_C13_wsumnorm"):          # one gradient alone: the other's loop trips and do_pts must not enter
        assert torch.equal(_splat_abi(c, neg, dfeat, idx, dist, dg, want_feat=False)[0], gp)
        assert torch.equal(_splat_abi(c, neg, dfeat, idx, dist, dg, want_pts=False)[1], gf)


# ---- the training quantiser ------------------------------------------------------------------------------------------------------------------
_VQ = {c.id: c for c in VR.ROUTE_CASES}


def _vq_abi(z, idx, embed, cluster_size, embed_avg, decay, eps, gq, gd):
    """The four entry points on given codes (int32, any value) -> dict of their outputs; every output asserted written everywhere and
    nowhere else, the workspace 0xff before each call that takes one"""
    N, D = z.shape
    K = embed.shape[1]
    rbuf = torch.full((K + 2, D), POISON, device=DEV)          # the codebook's rows between two rows of poison: a gather that takes
    rbuf[1:K + 1] = embed.t()                                  # code -1 or code K for a row instead of for zeros reads one
    rows = rbuf[1:K + 1]
    cbuf, counts = _guarded_int(K)
    sbuf, sums = _guarded(D * K)
    qbuf, quant = _guarded(N * D)
    dbuf, diff = _guarded(1)
    ebuf, new_embed = _guarded(D * K)
    gbuf, gi = _guarded(N * D)
    cs, avg = cluster_size.clone(), embed_avg.clone()
    ws = _workspace("ps_vq_train_workspace_bytes", N, D, K)
    _lib.call("ps_vq_train_stats_f32", z, idx, N, D, K, counts, sums, ws, ws.numel())
    ws.fill_(255)
    _lib.call("ps_vq_train_quantize_f32", z, idx, rows, N, D, K, quant, diff, ws, ws.numel())
    ws.fill_(255)
    _lib.call("ps_vq_train_update_f32", counts, sums, D, K, float(decay), 1 - float(decay), float(eps), cs, avg, new_embed, ws, ws.numel())
    _lib.call("ps_vq_train_backward_f32", z, idx, rows, gq, gd.reshape(1), N, D, K, gi)
    torch.cuda.synchronize()
    assert (counts != INT_FILL).all() and _untouched_int(cbuf, K) and all(torch.isfinite(t).all() for t in (sums, quant, diff, new_embed, gi, cs, avg))
    assert _untouched(sbuf, D * K) and _untouched(qbuf, N * D) and _untouched(dbuf, 1) and _untouched(ebuf, D * K) and _untouched(gbuf, N * D)
    return dict(counts=counts, sums=sums.view(D, K), quantize=quant.view(N, D), diff=diff.view(()), embed=new_embed.view(D, K),
                cluster_size=cs, embed_avg=avg, grad_input=gi.view(N, D))


def _vq_check_abi(name, z, idx, before, decay, eps, record):
    """_vq_abi against the fp64 formulas of tests/_vq_train_ref.py on a codebook with a zero row appended (for codes inside 0 .. K-1 it
    changes nothing) -> (the outputs, the expected values)"""
    N, D = z.shape
    K = before["embed"].shape[1]
    gen = torch.Generator().manual_seed(N + D + K)
    gq, gd = torch.randn(N, D, generator=gen).to(DEV), torch.tensor(-0.75, device=DEV)
    got = _vq_abi(z, idx.to(torch.int32).contiguous(), before["embed"], before["cluster_size"], before["embed_avg"], decay, eps, gq, gd)
    ext, idx_ext = VR.with_zero_row(before["embed"].cpu(), idx)
    pad = lambda t: torch.cat([t.cpu(), torch.zeros_like(t.cpu()[..., :1])], -1)
    exp = VR.expected(z, ext, idx_ext, pad(before["cluster_size"]), pad(before["embed_avg"]), decay, eps)
    assert torch.equal(got["counts"].cpu().long(), exp["counts"][:K]), f"{name}: counts"
    VR.check(f"{name} ABI sums", got["sums"], exp["sums"][:, :K], exp["bound"]["sums"][:, :K], record)
    zc = z.cpu()
    assert torch.equal(got["quantize"].cpu(), zc + (VR.gather(ext, idx_ext) - zc)), f"{name}: quantize is not torch's fp32 z + (e - z) bit for bit"
    VR.check(f"{name} ABI diff", got["diff"], exp["diff"], exp["bound"]["diff"], record)
    want, term = VR.grad_input(zc.double(), ext.double(), idx_ext, gq.cpu().double(), gd.cpu().double())
    VR.check(f"{name} ABI grad_input", got["grad_input"], want, VR.grad_bound(gq.cpu().double(), term), record)
    return got, exp


@pytest.mark.parametrize("case", VR.ROUTE_CASES, ids=lambda c: c.id)
def test_vq_route_against_fp64(case):
    N, D, K = case.shape
    p = VR.plan(N, D, K)
    assert p.bytes == _lib.call("ps_vq_train_workspace_bytes", N, D, K)
    name = f"{case.id} N{N} D{D} K{K}"
    record = {}
    q = vq_ops._quantizer(D, K)
    vq_ops._update(f"{name} first update", q, vq_ops._latents(N, D, 21))        # through Quantize in train mode, from an empty history
    before = vq_ops._state(q)
    z = vq_ops._latents(N, D, 22)
    exp, (quantize, diff, ind) = vq_ops._update(f"{name} second update", q, z)
    idx = ind.reshape(-1)
    assert int(exp["counts"].max()) > 1 and int((exp["counts"] > 0).sum()) > 1
    # the entry points themselves on the module's codes: the module's bits, the update's three buffers included
    got, _ = _vq_check_abi(name, z, idx, before, q.decay, q.eps, record)
    after = vq_ops._state(q)
    assert torch.equal(got["quantize"], quantize) and torch.equal(got["diff"], diff)
    assert all(torch.equal(got[k], after[k]) for k in ("embed", "cluster_size", "embed_avg"))
    print(f"{name} {p}: largest error / bound {record}")


def test_vq_codes_outside_the_codebook():
    """The header's contract: a code outside 0 .. K-1 selects a row of zeros in the gathers and counts for no code in the statistics"""
    N, D, K = _VQ["dt2"].shape
    q = vq_ops._quantizer(D, K)
    z = vq_ops._latents(N, D, 22)
    before = vq_ops._state(q)
    with torch.no_grad():
        idx = q.eval()(z)[2].reshape(-1).clone()
    gen = torch.Generator().manual_seed(5)
    bad = torch.randperm(N, generator=gen)[:15]                                  # about 3 % of the rows, five of each kind
    idx[bad.to(DEV)] = torch.tensor([-1, K, K + 7], device=DEV).repeat(5)
    assert (K + 7) // VR.TILE == K // VR.TILE                                    # (K and K + 7 are columns of the padded last code tile)
    record = {}
    got, exp = _vq_check_abi("codes outside the codebook", z, idx, before, q.decay, q.eps, record)
    assert int(got["counts"].sum()) == N - 15 and int(exp["counts"][K]) == 15
    zc = z.cpu()
    assert torch.equal(got["quantize"].cpu()[bad], zc[bad] + (0 - zc[bad]))
    inside = torch.ones(N, dtype=torch.bool)
    inside[bad] = False
    counts, sums = VR.stats(zc[inside].double(), idx.cpu()[inside], K)            # those rows add to no count and no sum
    assert torch.equal(got["counts"].cpu().long(), counts)
    VR.check("codes outside the codebook: sums of the other rows alone", got["sums"], sums, exp["bound"]["sums"][:, :K], record)
    print(f"codes outside the codebook: largest error / bound {record}")


# ---- the locally masked convolution, backward and forward --------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", LR.ROUTE_CASES, ids=lambda c: c.id)
def test_lmconv_route_against_fp64(case):
    B, Ci, Co, H, W, dil = case.shape
    p = LR.plan(B, Ci, Co, H, W)
    assert p.bytes == _lib.call("ps_lmconv_bwd_workspace_bytes", B, Ci, Co, H, W)
    x, m, w, b, g = LR.inputs(B, Ci, Co, H, W, seed=LR.ROUTE_CASES.index(case))
    name = f"{case.id} B{B} {Ci}->{Co} {H}x{W} d{dil} ({p.parts} parts of {p.chunk} steps, the last of {p.last})"
    assert all(bool(t.any()) for t in LR.bounds(x, m, w, g, dil)), "a gradient whose every bound is 0 proves nothing"
    _check_case(name, x, m, w, b, g, dil)
    y, gx, gw, gb = _hip_gradients(x, m, w, b, g, dil)
    y64, ybound = LR.forward64(x, m, w, b, dil)
    assert ybound.any()
    LR.check(f"{name} y", y, y64, ybound)
    if p.chunk != 6:
        return
    # ps_lmconv_grad_weight_f32 itself: every element written, none outside, the module's bits
    wbuf, gw2 = _guarded(Co * Ci * 9)
    bbuf, gb2 = _guarded(Co)
    ws = _workspace("ps_lmconv_bwd_workspace_bytes", B, Ci, Co, H, W)
    _lib.call("ps_lmconv_grad_weight_f32", x.to(DEV), g.to(DEV), m.to(DEV), 9 * H * W, B, Ci, Co, H, W, dil, gw2, gb2, ws, ws.numel())
    torch.cuda.synchronize()
    assert torch.isfinite(gw2).all() and torch.isfinite(gb2).all() and _untouched(wbuf, Co * Ci * 9) and _untouched(bbuf, Co)
    assert torch.equal(gw2.view(Co, Ci, 3, 3), gw) and torch.equal(gb2, gb)
