"""GPU: the splits, walks, rows and strides of csrc/thin_train.hip that tests/test_thin_train_gpu.py never takes, on the route cases of
tests/_thin_train_ref.py (tests/test_thin_routes_cpu.py asserts, without a GPU, that every case reaches its branch and that no shape of
the operator tests does).  A case the Functions take goes through the operator tests' own bodies -- their checks and derived bounds
unchanged.  A case they refuse goes through the C ABI with every output NaN-filled inside rims of sentinel floats and the workspace's
every byte 0xff inside rims of its own, against the fp64 formulas under the same bounds: an element left unwritten, a store outside an
output and a slab read before it was written all show.  Exact results where the arithmetic leaves no choice: one-hot operands on frames
of 1 x 4 to 5 x 12 and in the last pixel of a capped split, and ps_thin_add_bias_f32 bit for bit on flat buffers.  Every check prints its
error / bound; docs/LAB_NOTEBOOK.md has the table per case."""
import pytest
import torch

import _thin_train_ref as ref
import test_thin_train_gpu as ops
from pixelsynth_amd import _lib
from test_thin_train_gpu import _backward, _rule
from test_train_routes_gpu import GUARD, SENTINEL, _guarded, _untouched

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_by_via = lambda via: [r for r in ref.ROUTES if r.via == via]  # noqa: E731


# ---- through the Functions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("route", _by_via("function"), ids=repr)
def test_a_function_route(route):
    """The body of test_a_thin_out_layer / test_a_thin_in_layer at the route's shape: the forward bits, expand_bound, sums_bound and the
    project's rule for all three gradients, two runs, the last frame alone"""
    r = route
    try:
        if r.kind == "out":
            ops.test_a_thin_out_layer(r.frame, r.wide, r.T, r.k)
        else:
            ops.test_a_thin_in_layer(r.frame, r.wide, r.k)
    finally:
        ops._REFS.pop((r.kind, r.frame, r.wide, r.T, r.k), None)          # (the capped cases' references: tens of megabytes, used here alone)


# ---- through the C ABI ----------------------------------------------------------------------------------------------------------------------
def _flat(t):
    """(B, C, H, W) on the host -> (B, H, W, C) on the device, contiguous"""
    return t.permute(0, 2, 3, 1).contiguous().to(DEV)


def _abi_grad_weight(x, w, g, wide_is_g, with_bias=True):
    """ps_thin_grad_weight_f32 on the layer x (B, Ci, H, W), w (Co, Ci, k, k), g (B, Co, H, W) of the host, the thin side x (wide_is_g) or
    g -> (grad_weight (Co, Ci, k, k), grad_bias (Co) or None, the first slab's weight sums as the entry point lays them out, its bias sums
    rounded).  Every output and the workspace asserted written nowhere outside."""
    B, _, H, W = x.shape
    k = w.size(2)
    thin, wide = (x, g) if wide_is_g else (g, x)
    T, Cw = thin.size(1), wide.size(1)
    nw, nb = k * k * T * Cw, (Cw if wide_is_g else T)
    need = _lib.call("ps_thin_train_workspace_bytes", B, H, W, Cw, T, k)
    assert need == ref.workspace_bytes(B, H, W, Cw, T, k) and need % 4 == 0
    wbuf, gw = _guarded(nw)
    bbuf, gb = _guarded(nb)
    sbuf, ws = _guarded(need // 4)
    ws.view(torch.uint8).fill_(255)
    _lib.call("ps_thin_grad_weight_f32", _flat(thin), _flat(wide), B, H, W, Cw, T, k, int(wide_is_g), gw, gb if with_bias else None, ws, need)
    torch.cuda.synchronize()
    assert _untouched(wbuf, nw) and _untouched(bbuf, nb) and _untouched(sbuf, need // 4) and torch.isfinite(gw).all()
    assert torch.isfinite(gb).all() if with_bias else torch.isnan(gb).all()          # NULL: nothing is written beyond grad_weight
    slab_b = ws[nw:nw + 2 * Cw].view(torch.float64)[:nb].float() if with_bias else None
    out = gw.view(k, k, T, Cw)
    return (out.permute(3, 2, 0, 1) if wide_is_g else out.permute(2, 3, 0, 1)).contiguous(), gb if with_bias else None, ws[:nw].clone(), slab_b


def _abi_expand(w, g):
    """ps_thin_expand_f32 on w (T, Cw, k, k), g (B, T, H, W) of the host -> grad_input (B, Cw, H, W), a view of the (B, H, W, Cw) output"""
    B, T, H, W = g.shape
    Cw, k = w.size(1), w.size(2)
    obuf, out = _guarded(B * H * W * Cw)
    _lib.call("ps_thin_expand_f32", _flat(g), w.flip(2, 3).permute(2, 3, 0, 1).contiguous().to(DEV), B, H, W, T, Cw, k, out)
    torch.cuda.synchronize()
    assert _untouched(obuf, B * H * W * Cw) and torch.isfinite(out).all()
    return out.view(B, H, W, Cw).permute(0, 3, 1, 2)


@pytest.mark.parametrize("route", _by_via("grad_weight"), ids=repr)
def test_a_grad_weight_route_against_fp64(route):
    """Both values of wide_is_g, every T and k, grad_bias given and NULL: sums_bound and the project's rule; with one part the second kernel
    copies the slab"""
    r = route
    parts = len(ref.part_ranges(r.npix))
    worst = {"grad_weight": 0.0, "grad_bias": 0.0, "rule": 0.0}
    for wide_is_g in (0, 1):
        for T in ref.ABI_T:
            for k in ref.ABI_K:
                Ci, Co = (T, r.wide) if wide_is_g else (r.wide, T)
                x, w, b, g = ref.layer_inputs(Ci, Co, r.frame, k)
                g64, g32 = ref.conv_grads(x, w, b, g), ref.conv_grads(x, w, b, g, torch.float32)
                assert _lib.call("ps_thin_train_parts", *r.frame, r.wide, T, k) == parts
                tag = f"{r.id} wide_is_g = {wide_is_g}, T = {T}, k = {k}:"
                gw, gb, slab_w, slab_b = _abi_grad_weight(x, w, g, wide_is_g)
                bw, bb = ref.sums_bound(x, w, g)
                rw = ref.check(f"{tag} grad_weight, (L + parts) u sum |g||x| (L = {ref.chain(r.npix)}, parts = {parts})", gw, g64[1], bw)
                rb = ref.check(f"{tag} grad_bias, (L + parts) u sum |g|", gb, g64[2], bb)
                assert rw <= 1.0 and rb <= 1.0, tag
                rule = max(_rule(f"{tag} grad_weight, the project's rule", gw, g64[1], g32[1]), _rule(f"{tag} grad_bias, the project's rule", gb, g64[2], g32[2]))
                worst = {"grad_weight": max(worst["grad_weight"], rw), "grad_bias": max(worst["grad_bias"], rb), "rule": max(worst["rule"], rule)}
                if parts == 1:
                    assert torch.equal(slab_w, (gw.permute(2, 3, 1, 0) if wide_is_g else gw.permute(2, 3, 0, 1)).reshape(-1)) and torch.equal(slab_b, gb)
                alone, none = _abi_grad_weight(x, w, g, wide_is_g, with_bias=False)[:2]
                assert none is None and torch.equal(alone, gw), tag
                assert torch.equal(_abi_grad_weight(x, w, g, wide_is_g)[0], gw), tag          # two runs, the same bits
    print(f"{r.id}: largest error / bound", ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))


@pytest.mark.parametrize("route", _by_via("expand"), ids=repr)
def test_an_expand_route_against_fp64(route):
    """Every T and k: expand_bound and the project's rule; the last frame alone gives the batch's bits"""
    r = route
    worst = {"grad_input": 0.0, "rule": 0.0}
    for T in ref.ABI_T:
        for k in ref.ABI_K:
            x, w, b, g = ref.layer_inputs(r.wide, T, r.frame, k)
            g64, g32 = ref.conv_grads(x, w, b, g)[0], ref.conv_grads(x, w, b, g, torch.float32)[0]
            tag = f"{r.id} T = {T}, k = {k}:"
            gx = _abi_expand(w, g)
            ri = ref.check(f"{tag} grad_input, n u sum |w g|", gx, g64, ref.expand_bound(x, w, g))
            assert ri <= 1.0, tag
            worst = {"grad_input": max(worst["grad_input"], ri), "rule": max(worst["rule"], _rule(f"{tag} grad_input, the project's rule", gx, g64, g32))}
            assert torch.equal(_abi_expand(w, g[-1:])[0], gx[-1]) and torch.equal(_abi_expand(w, g), gx), tag
    print(f"{r.id}: largest error / bound", ", ".join(f"{n} {v:.3f}" for n, v in worst.items()))


# ---- exact results ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 4), (3, 4)], ids=lambda v: str(v))
def test_a_one_hot_gradient_at_every_pixel_returns_the_weights_themselves(H, W):
    """ps_thin_expand_f32 where one thread's window holds both borders of the frame: g one-hot at pixel f of frame f, for every pixel --
    grad_input is W[j][c][dy + r][dx + r] at (Y + dy, X + dx) where that is inside the frame and 0 elsewhere, exactly"""
    B, wide = H * W, 32
    for T, k in ((1, 3), (2, 3), (3, 3), (4, 3), (2, 1)):
        r, j = k // 2, T - 1
        x, w, b, _ = ref.layer_inputs(wide, T, (B, H, W), k, seed=3)
        g, want = torch.zeros(B, T, H, W), torch.zeros(B, wide, H, W)
        for f in range(B):
            Y, X = divmod(f, W)
            g[f, j, Y, X] = 1.0
            for dy in range(-r, r + 1):
                for dx in range(-r, r + 1):
                    if 0 <= Y + dy < H and 0 <= X + dx < W:
                        want[f, :, Y + dy, X + dx] = w[j, :, dy + r, dx + r]
        gx = _abi_expand(w, g).cpu()
        assert torch.equal(gx, want) and torch.equal(gx.double(), ref.conv_grads(x, w, b, g)[0]), (T, k)


def _unflat(p, H, W):
    return p // (H * W), (p // W) % H, p % W


@pytest.mark.parametrize("wide_is_g", [0, 1])
@pytest.mark.parametrize("frame", [(2, 3, 4), (4, 3, 4), (3, 5, 12)], ids=lambda f: "x".join(map(str, f)))
def test_one_hot_pairs_give_an_exact_product_in_the_right_tap(frame, wide_is_g):
    """ps_thin_grad_weight_f32 on frames whose walk is no (32, 0) -- in 4 x 3 x 4 the last pixels are their threads' second, reached by a
    step that passes 2 H --: x one-hot (3.0) at P and g one-hot (0.5) at Q -- grad_weight is 1.5 in the tap that leads from Q to P and 0
    everywhere else, for every P within a row and a pixel of Q in memory: also where they are neighbours in memory only (across a row end,
    across a frame end); grad_bias is 0.5 in g's channel"""
    B, H, W = frame
    npix, wide, T = B * H * W, 32, 3
    Ci, Co = (T, wide) if wide_is_g else (wide, T)
    ci, co = Ci - 1, Co - 2
    w = torch.zeros(Co, Ci, 3, 3)
    taps, strangers = 0, 0
    for q in sorted({0, W - 1, W, H * W - 1, H * W, H * W + W + 1, npix - W, npix - 1}):
        for d in (-W - 1, -W, -W + 1, -1, 0, 1, W - 1, W, W + 1):
            p = q + d
            if not 0 <= p < npix:
                continue
            (fq, yq, xq), (fp, yp, xp) = _unflat(q, H, W), _unflat(p, H, W)
            x, g = torch.zeros(B, Ci, H, W), torch.zeros(B, Co, H, W)
            x[fp, ci, yp, xp], g[fq, co, yq, xq] = 3.0, 0.5
            want, want_b = torch.zeros_like(w), torch.zeros(Co)
            want_b[co] = 0.5
            if fp == fq and abs(yp - yq) <= 1 and abs(xp - xq) <= 1:
                want[co, ci, yp - yq + 1, xp - xq + 1] = 1.5
                taps += 1
            else:
                strangers += 1
            gw, gb = _abi_grad_weight(x, w, g, wide_is_g)[:2]
            assert torch.equal(gw.cpu(), want) and torch.equal(gb.cpu(), want_b), (q, p)
            assert torch.equal(want.double(), ref.conv_grads(x, w, torch.zeros(Co), g)[1])
    assert taps > 20 and strangers > 10


def test_a_one_hot_in_the_last_pixel_of_a_capped_split_lands_in_the_right_tap():
    """capped-ragged through conv_thin_out_train: the last pixel lies in the last part, 128 pixels behind 252 parts of 1056.  x one-hot there
    and g one row and one pixel before it, then the other way round: 1.5 in tap (2, 2), then in tap (0, 0), and nothing else"""
    r = next(r for r in ref.ROUTES if r.id == "capped-ragged")
    B, H, W = r.frame
    lo, hi = ref.part_ranges(r.npix)[-1]
    assert hi - lo == 128 and lo == 252 * 1056 and hi - 1 == (H - 1) * W + W - 1
    w, b = torch.zeros(r.T, r.wide, 3, 3), torch.zeros(r.T)
    ci, co = r.wide - 1, r.T - 2
    for last_is_x, tap in ((True, (2, 2)), (False, (0, 0))):
        x, g = torch.zeros(B, r.wide, H, W), torch.zeros(B, r.T, H, W)
        P, Q = ((H - 1, W - 1), (H - 2, W - 2)) if last_is_x else ((H - 2, W - 2), (H - 1, W - 1))
        x[0, ci, P[0], P[1]], g[0, co, Q[0], Q[1]] = 3.0, 0.5
        _, _, gw, gb = _backward("out", x, w, b, g, (False, True, True))
        want, want_b = torch.zeros_like(w), torch.zeros(r.T)
        want[co, ci, tap[0], tap[1]], want_b[co] = 1.5, 0.5
        assert torch.equal(gw.cpu(), want) and torch.equal(gb.cpu(), want_b), tap


# ---- the bias of a forward pass -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c, _ in ref.BIAS_ROUTES], ids=lambda c: f"{c[0]}x{c[1]}{'' if c[2] else '-off4'}")
def test_add_bias_on_flat_buffers_bit_for_bit(case):
    """ps_thin_add_bias_f32 against y + bias[c] of the host, one rounded add: the grid-stride loops' second pass, the scalar kernel at a
    C that is a multiple of 4 (y four bytes off a multiple of 16), C = 5, one element"""
    npix, C, aligned = case
    n, off = npix * C, 0 if aligned else 1
    gen = torch.Generator().manual_seed(npix + C)
    y0, bias = torch.randn(npix, C, generator=gen), torch.randn(C, generator=gen)
    buf = torch.full((GUARD + off + n + GUARD,), SENTINEL, device=DEV)
    y = buf[GUARD + off:GUARD + off + n]
    y.copy_(y0.view(-1))
    bd = bias.to(DEV)
    assert (y.data_ptr() % 16 == 0) == aligned and bd.data_ptr() % 16 == 0
    _lib.call("ps_thin_add_bias_f32", y, bd, npix, C)
    torch.cuda.synchronize()
    assert torch.equal(y.cpu().view(npix, C), y0 + bias)
    assert bool((buf[:GUARD + off] == SENTINEL).all() and (buf[GUARD + off + n:] == SENTINEL).all())
