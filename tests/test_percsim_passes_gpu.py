"""GPU: ps_percsim_input, ps_percsim_tap and ps_percsim_finish (csrc/percsim.hip) called on their own, off the shapes VGG16 and
PNet.hip_takes happen to give them.

Exact: every case of tests/_percsim_pass_cases.py on integer_maps (every fp32 sum of the tap is exact) against the fp64 reference:
a layer's score within 2^-24 of float32(scores64) and the total within 2^-21 -- what is left is the order of the fp64 steps (1e-13)
and the one rounding to fp32 of a value in [0, 1] and of a sum in [0, 5].  Rounding: the same on float_maps within the worst case of
the kernel's own summation (_percsim_pass_cases.rounding_bound).  The pool: max_pool2d of the RAW map bit for bit, inside a buffer
whose neighbouring rows keep a sentinel; the scores do not depend on whether it is written.  A pass of three pairs has the bits of
three passes of one.  The workspace's size in closed form, its layout (the finish alone on a workspace written by the header's
layout) and the bytes behind it.  Non-finite values as torch.relu and F.max_pool2d hand them on.  The input pass bit for bit against
the same fp32 operations in torch on the CPU, into slices of one buffer as perceptual._passes lays them out.  Every refusal of the
three entry points, with the outputs left alone.

Measured on the MI355X: MEASURED below."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _percsim_pass_cases as E
from pixelsynth_amd import _images, _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
SENTINEL = -1234.5
NAN, INF = float("nan"), float("inf")
PLAIN, VIS, INVIS, RAW = 0, 1, 2, 3
GUARD = 32                                # doubles behind the workspace
WS_FILL = -0x000A5A5A5A5A5A5B             # an int64 whose bits are a NaN: a tile no tap wrote makes its score NaN
MEASURED = """one run on the MI355X:
exact, all 24 cases: every layer score and every total equal to float32(scores64), difference 0
rounding, the largest error of a layer's score over all cases, per C (of its bound, ratio): C = 64 2.844e-08 of 1.132e-06 (0.025),
C = 128 2.806e-08 of 1.609e-06 (0.017), C = 192 2.891e-08 of 2.086e-06 (0.014), C = 256 2.848e-08 of 2.563e-06 (0.011),
C = 320 2.903e-08 of 3.040e-06 (0.010), C = 512 2.936e-08 of 4.470e-06 (0.007); the total 2.361e-07 of 5.305e-06 at most (0.045, a case
off the network's channels) and 1.135e-07 of 1.425e-05 on the network's.  Every maximum is the score's own rounding to fp32
(2^-25 = 2.98e-08): the sums' errors average out far below their worst case."""


def t(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the cases' maps are shared and read-only)


def bits(a):
    return a.contiguous().view(torch.int32)


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(bits(a), bits(b))


def equal_or_both_nan(a, b):
    return a.shape == b.shape and bool(((a == b) | (a.isnan() & b.isnan())).all())


def nchw(y):
    return y.permute(0, 3, 1, 2)


def max_pool(y):
    """F.max_pool2d(2, 2) of an NHWC map on the CPU -> NHWC"""
    return F.max_pool2d(nchw(y), 2, 2).permute(0, 2, 3, 1).contiguous()


def run_pass(maps, P, H, W, pool=True):
    """The taps of `maps` {layer: (2P, Hl, Wl, C) tensor on the device} and the finish, the workspace's other blocks zero ->
    (layers (P, 5), total (P,), {layer: pooled}) on the CPU.  The pooled maps, the scores and the workspace lie inside larger
    buffers: what surrounds them must keep its fill."""
    torch.cuda.set_device(DEV)
    need = _lib.call("ps_percsim_workspace_bytes", P, H, W)
    assert need == E.workspace_bytes(P, H, W)
    ws = torch.full((need // 8 + GUARD,), WS_FILL, dtype=torch.int64, device=DEV)
    assert bool(ws.view(torch.float64).isnan().all())
    for l in set(range(E.LAYERS)) - set(maps):
        o = E.layer_offset(P, H, W, l)
        ws[o:o + P * E.tiles_of(H, W, l)] = 0
    pooled = {}
    for l, y in maps.items():
        N, Hl, Wl, C = y.shape
        buf = torch.full((N + 2, Hl // 2, Wl // 2, C), SENTINEL, device=DEV) if pool else None
        _lib.call("ps_percsim_tap", y, P, H, W, l, C, None if buf is None else buf[1:-1], ws, need)
        if pool:
            assert bool((buf[0] == SENTINEL).all()) and bool((buf[-1] == SENTINEL).all()), ("around pooled", l)
            pooled[l] = buf[1:-1].cpu()
    layers = torch.full((P + 2, E.LAYERS), SENTINEL, device=DEV)
    total = torch.full((P + 2,), SENTINEL, device=DEV)
    _lib.call("ps_percsim_finish", ws, need, P, H, W, layers[1:-1], total[1:-1])
    assert bool((layers[[0, -1]] == SENTINEL).all()) and bool((total[[0, -1]] == SENTINEL).all()), "around the scores"
    assert bool((ws[need // 8:] == WS_FILL).all()), "behind the workspace"
    return layers[1:-1].cpu(), total[1:-1].cpu(), pooled


def on_device(maps):
    return {l: t(y) for l, y in maps.items()}


def index_of(H, W, P, chans=None):
    return E.CASES.index((H, W, P, chans or dict(enumerate(E.NET_C))))


IDS = [E.name(c) for c in E.CASES]


# ---- tap and finish
@pytest.mark.parametrize("k", range(len(E.CASES)), ids=IDS)
def test_tap_and_finish_exact_on_integer_maps(k):
    H, W, P, chans = E.CASES[k]
    maps = E.integer_maps(k)
    want_layers, want_total = E.scores64(maps, P)
    dev = on_device(maps)
    layers, total, pooled = run_pass(dev, P, H, W)
    d_layer = np.abs(layers.double().numpy() - want_layers.astype(np.float32).astype(np.float64))
    d_total = np.abs(total.double().numpy() - want_total.astype(np.float32).astype(np.float64))
    print(f"exact {E.name(E.CASES[k])}: layers off float32(fp64) by {d_layer.max():.3e}, total by {d_total.max():.3e}")
    assert (d_layer <= 2.0 ** -24).all(), d_layer
    assert (d_total <= 2.0 ** -21).all(), d_total
    for l in set(range(E.LAYERS)) - set(chans):
        assert bool((layers[:, l] == 1.0).all()), "a layer that was not tapped"
    for l, y in maps.items():
        want = torch.from_numpy(E.pool(y))
        assert same_bits(pooled[l], want), ("pooled", l)
        for pair, spot in E.forced_spots(E.CASES[k], l).items():
            r, c = spot["negative_window"]
            got = pooled[l][[pair, P + pair], r // 2, c // 2, (7 * pair + 5) % chans[l]]
            assert got.tolist() == [-1.0, -1.0], "the pool is of the map before its ReLU"
    no_pool = run_pass(dev, P, H, W, pool=False)
    assert same_bits(no_pool[0], layers) and same_bits(no_pool[1], total), "the scores do not depend on pooled"


@pytest.mark.parametrize("k", range(len(E.CASES)), ids=IDS)
def test_tap_and_finish_rounding_on_float_maps(k):
    H, W, P, chans = E.CASES[k]
    maps = E.float_maps(k)
    want_layers, want_total = E.scores64(maps, P)
    dev = on_device(maps)
    layers, total, pooled = run_pass(dev, P, H, W)
    err = np.abs(layers.double().numpy() - want_layers).max(0)
    err_total = float(np.abs(total.double().numpy() - want_total).max())
    # the total: the tapped layers' bounds, and 2^-24 for each of the others (the share of the total's own rounding that a tapped
    # layer's bound holds as its last term)
    bound_total = sum(E.rounding_bound(C) for C in chans.values()) + (E.LAYERS - len(chans)) * 2.0 ** -24
    worst = {}
    for l, C in chans.items():
        worst[C] = max(worst.get(C, 0.0), float(err[l]))
    print(f"rounding {E.name(E.CASES[k])}: " + ", ".join(f"C = {C} {e:.3e} of {E.rounding_bound(C):.3e} ({e / E.rounding_bound(C):.3f})"
                                                          for C, e in sorted(worst.items()))
          + f"; total {err_total:.3e} of {bound_total:.3e} ({err_total / bound_total:.3f})")
    for l in range(E.LAYERS):
        if l in chans:
            assert err[l] <= E.rounding_bound(chans[l]), (l, err[l])
            assert 0.25 < float(layers[:, l].min()) and float(layers[:, l].max()) < 1.0
        else:
            assert bool((layers[:, l] == 1.0).all())
    assert err_total <= bound_total, err_total
    for l, y in maps.items():
        assert same_bits(pooled[l], max_pool(torch.from_numpy(np.array(y)))), ("pooled", l)
    no_pool = run_pass(dev, P, H, W, pool=False)
    assert same_bits(no_pool[0], layers) and same_bits(no_pool[1], total), "the scores do not depend on pooled"


def test_one_tap_on_a_zero_workspace():
    k = index_of(128, 384, 3)
    y = E.integer_maps(k)[2]
    layers, total, _ = run_pass({2: t(y)}, 3, 128, 384)
    want = (1.0 - E.tap64(y, 3)).astype(np.float32)
    assert bool((layers[:, [0, 1, 3, 4]] == 1.0).all()), "the four layers nobody tapped"
    assert np.abs(layers[:, 2].double().numpy() - want.astype(np.float64)).max() <= 2.0 ** -24
    assert np.abs(total.double().numpy() - (4.0 + (1.0 - E.tap64(y, 3)))).max() <= 2.0 ** -21


def test_three_pairs_have_the_bits_of_three_single_passes():
    H, W, P = 128, 384, 3
    maps = on_device(E.float_maps(index_of(H, W, P)))
    layers, total, pooled = run_pass(maps, P, H, W)
    assert same_bits(run_pass(maps, P, H, W)[0], layers), "run to run"
    assert len(set(total.tolist())) == P
    for i in range(P):
        one = {l: y[[i, P + i]].contiguous() for l, y in maps.items()}
        l1, t1, p1 = run_pass(one, 1, H, W)
        assert same_bits(l1, layers[i:i + 1]) and same_bits(t1, total[i:i + 1]), i
        for l in maps:
            assert same_bits(p1[l], pooled[l][[i, P + i]]), (i, l)


# ---- the workspace
def test_workspace_bytes_in_closed_form():
    for H, W in E.SIZES:
        for P in (1, 3, 65535):
            tiles = sum((H >> l) * (W >> l) // 64 for l in range(5))
            assert _lib.call("ps_percsim_workspace_bytes", P, H, W) == 8 * P * tiles == E.workspace_bytes(P, H, W), (P, H, W)
    for bad in (0, 64, 192, 200):
        assert _lib.call("ps_percsim_workspace_bytes", 1, bad, 128) == 0 and _lib.call("ps_percsim_workspace_bytes", 1, 128, bad) == 0
    assert _lib.call("ps_percsim_workspace_bytes", 0, 128, 128) == 0


@pytest.mark.parametrize("H,W", E.SIZES)
def test_finish_alone_on_the_documented_layout(H, W):
    torch.cuda.set_device(DEV)
    P = 3
    host = E.finish_workspace(P, H, W)
    want_layers, want_total = E.finish64(host, P, H, W)
    ws = t(host)
    assert ws.dtype == torch.float64 and ws.numel() * 8 == _lib.call("ps_percsim_workspace_bytes", P, H, W)
    layers, total = torch.full((P, 5), SENTINEL, device=DEV), torch.full((P,), SENTINEL, device=DEV)
    _lib.call("ps_percsim_finish", ws, ws.numel() * 8, P, H, W, layers, total)
    assert np.array_equal(layers.cpu().numpy(), want_layers), (layers.cpu().numpy() - want_layers)
    assert np.array_equal(total.cpu().numpy(), want_total)
    assert np.array_equal(ws.cpu().numpy(), host), "the finish only reads"


# ---- non-finite values
NF = dict(H=128, W=128, P=3, layer=2, row=5, col=7, channel=77)      # (channel 77: the second trip of lane 3's loop)


@pytest.fixture(scope="module")
def clean_pass():
    maps = on_device(E.float_maps(index_of(NF["H"], NF["W"], NF["P"])))
    return maps, run_pass(maps, NF["P"], NF["H"], NF["W"])


def with_value(maps, image, value):
    y = maps[NF["layer"]].clone()
    y[image, NF["row"], NF["col"], NF["channel"]] = value
    return {**maps, NF["layer"]: y}


@pytest.mark.parametrize("image", [NF["P"] + 1, 1], ids=["in1", "in0"])
@pytest.mark.parametrize("value", [NAN, INF], ids=["nan", "inf"])
def test_a_nan_or_inf_reaches_its_layer_and_its_pair_alone(clean_pass, value, image):
    maps, (layers, total, pooled) = clean_pass
    P, layer = NF["P"], NF["layer"]
    dirty = with_value(maps, image, value)
    got_layers, got_total, got_pooled = run_pass(dirty, P, NF["H"], NF["W"])
    hit = torch.zeros(P, 5, dtype=torch.bool)
    hit[1, layer] = True
    assert torch.equal(got_layers.isnan(), hit), got_layers
    assert torch.equal(got_total.isnan(), hit.any(1)), got_total
    assert same_bits(torch.where(hit, layers, got_layers), layers) and same_bits(torch.where(hit.any(1), total, got_total), total)
    for l in pooled:
        want = max_pool(dirty[l].cpu())
        assert int(want.isnan().sum()) == (l == layer and value != value)
        assert torch.equal(got_pooled[l].isnan(), want.isnan()), l
        assert equal_or_both_nan(got_pooled[l], want), l
        moved = bits(got_pooled[l]) != bits(pooled[l])
        assert int(moved.sum()) == (l == layer) and (l != layer or bool(moved[image, NF["row"] // 2, NF["col"] // 2, NF["channel"]]))


def test_minus_infinity_is_a_negative_value(clean_pass):
    maps, _ = clean_pass
    P, H, W, layer = NF["P"], NF["H"], NF["W"], NF["layer"]
    outs = []
    for value in (-INF, -1.0):
        y = with_value(maps, P + 1, value)[layer]
        y[0, 2:4, 8:10, 3] = value                    # a whole pool window of one channel
        y[P + 2, 9, 1, :] = value                     # a whole pixel: a zero norm
        outs.append((y, run_pass({layer: y}, P, H, W)))
    (y, (layers, total, pooled)), (_, (layers1, total1, _)) = outs
    assert bool(layers.isfinite().all()) and bool(total.isfinite().all())
    assert same_bits(layers, layers1) and same_bits(total, total1), "relu(-inf) = relu(-1) = 0"
    want = E.scores64({layer: y.cpu().numpy()}, P)[0]
    assert np.abs(layers.double().numpy() - want).max() <= E.rounding_bound(256)
    assert same_bits(pooled[layer], max_pool(y.cpu())) and float(pooled[layer][0, 1, 4, 3]) == -INF


# ---- the input pass
SHIFT = torch.tensor([-0.030, -0.088, -0.188], dtype=torch.float32).view(1, 3, 1, 1)
SCALE = torch.tensor([0.458, 0.448, 0.450], dtype=torch.float32).view(1, 3, 1, 1)


def input_mirror(img, mask, mode):
    """The header's fp32 operations in its order, in torch on the CPU: img (B, 3, H, W) fp32 or uint8 -> (B, H, W, 4) fp32"""
    u = img.float() / 255.0 if img.dtype == torch.uint8 else img
    if mode == VIS:
        u = u * mask
    elif mode == INVIS:
        u = u * (1.0 - mask)
    if mode != RAW:
        u = u * 2.0 - 1.0
    o = (u - SHIFT) / SCALE
    assert o.dtype == torch.float32
    return torch.cat([o, torch.zeros_like(o[:, :1])], 1).permute(0, 2, 3, 1).contiguous()


def stored(a, how, rng):
    """The CPU tensor a (B, 3, H, W) on the device as contiguous NCHW, as channels-last storage, or as the view [:, :, 1:-1, ::2] of
    a larger tensor of other values (a storage offset, a column stride of 2)"""
    if how == "nchw":
        return a.to(DEV)
    if how == "nhwc":
        x = a.to(DEV).permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2)
        assert x.stride(1) == 1
        return x
    B, C, H, W = a.shape
    big = torch.from_numpy(rng.integers(0, 256, size=(B, C, H + 2, 2 * W))).to(a.dtype)
    if a.dtype == torch.float32:
        big = big / 255.0 + 0.001
    big[:, :, 1:-1, ::2] = a
    x = big.to(DEV)[:, :, 1:-1, ::2]
    assert x.storage_offset() == 2 * W and x.stride(3) == 2 and torch.equal(x.cpu(), a)
    return x


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("H,W", [(1, 1), (3, 5), (17, 31), (256, 2)])
def test_input_pass_bit_for_bit(H, W, B):
    torch.cuda.set_device(DEV)
    rng = np.random.default_rng([H, W, B])
    n8 = B * 3 * H * W
    img8 = [torch.from_numpy(rng.permutation(np.arange(n8) % 256).astype(np.uint8).reshape(B, 3, H, W)) for _ in range(2)]
    if n8 >= 256:
        assert all(len(np.unique(i.numpy())) == 256 for i in img8), "every uint8 value"
    img32 = [torch.from_numpy(rng.random((B, 3, H, W), dtype=np.float32)) for _ in range(2)]
    raw32 = [i * 2 - 1 for i in img32]
    r = rng.random((B, 1, H, W))
    frac = torch.from_numpy(np.where(r < 0.25, 0.0, np.where(r > 0.75, 1.0, rng.random((B, 1, H, W)))).astype(np.float32))
    zeros, ones = torch.zeros(B, 1, H, W), torch.ones(B, 1, H, W)
    runs = [(PLAIN, img32, None), (PLAIN, img8, None), (RAW, raw32, None)]
    for m in (frac, zeros, ones):
        runs += [(VIS, img32, m), (VIS, img8, m), (INVIS, img32, m), (INVIS, img8, m)]
    layouts = ("nchw", "nhwc", "view")
    V, P = 3, 3 * B
    got = {}
    for j, (mode, (a, b), m) in enumerate(runs):
        for s in range(3):
            xa, xb = stored(a, layouts[s], rng), stored(b, layouts[(s + 1 + j) % 3], rng)
            v = (j + s) % V                          # the mode's place in the pass's buffer, as perceptual._passes cuts it
            x = torch.full((2 * P, H, W, 4), SENTINEL, device=DEV)
            _lib.call("ps_percsim_input", xa, _images.strides(xa), xb, _images.strides(xb), _images.DTYPES[a.dtype],
                      None if m is None else m.to(DEV), mode, B, H, W, x[v * B:(v + 1) * B], x[P + v * B:P + (v + 1) * B])
            x = x.cpu()
            out0, out1 = x[v * B:(v + 1) * B], x[P + v * B:P + (v + 1) * B]
            what = (mode, str(a.dtype), layouts[s], None if m is None else float(m.mean()))
            assert same_bits(out0, input_mirror(a, m, mode)) and same_bits(out1, input_mirror(b, m, mode)), what
            assert bool((bits(out0[..., 3]) == 0).all()) and bool((bits(out1[..., 3]) == 0).all()), "channel 3 is +0.0"
            written = torch.zeros(2 * P, dtype=torch.bool)
            written[v * B:(v + 1) * B] = written[P + v * B:P + (v + 1) * B] = True
            assert bool((x[~written] == SENTINEL).all()), what
        got[j] = out0
    # a mask of exact zeros in INVIS, of ones in VIS: the unmasked image's bits
    index = {(mode, a[0].dtype, None if m is None else id(m)): j for j, (mode, a, m) in enumerate(runs)}
    for dtype in (torch.float32, torch.uint8):
        plain = got[index[PLAIN, dtype, None]]
        assert same_bits(got[index[INVIS, dtype, id(zeros)]], plain) and same_bits(got[index[VIS, dtype, id(ones)]], plain)
        assert same_bits(got[index[VIS, dtype, id(zeros)]], got[index[INVIS, dtype, id(ones)]])


# ---- refusals
def test_refusals_leave_the_outputs_untouched():
    torch.cuda.set_device(DEV)
    need = _lib.call("ps_percsim_workspace_bytes", 1, 128, 128)
    y = torch.ones(2, 8, 8, 64, device=DEV)
    odd = torch.ones(2 * 8 * 8 * 64 + 4, device=DEV)                    # odd[1:] holds any map here, 4 bytes off a 16-byte boundary
    ws = torch.full((need // 8,), WS_FILL, dtype=torch.int64, device=DEV)
    pooled = torch.full((2, 4, 4, 64), SENTINEL, device=DEV)
    layers, total = torch.full((1, 5), SENTINEL, device=DEV), torch.full((1,), SENTINEL, device=DEV)

    def tap(y=y, P=1, H=128, W=128, layer=4, C=64, pooled=pooled, ws=ws, nbytes=need):
        _lib.call("ps_percsim_tap", y, P, H, W, layer, C, pooled, ws, nbytes)

    def finish(ws=ws, nbytes=need, P=1, H=128, W=128, layers=layers, total=total):
        _lib.call("ps_percsim_finish", ws, nbytes, P, H, W, layers, total)

    img = torch.full((1, 3, 4, 4), 0.5, device=DEV)
    img8 = torch.full((1, 3, 4, 4), 128, dtype=torch.uint8, device=DEV)
    mask = torch.ones(1, 1, 4, 4, device=DEV)
    out = torch.full((2, 4, 4, 4), SENTINEL, device=DEV)
    st = (ctypes.c_int64 * 4)(48, 16, 4, 1)

    def inp(a=img, sa=st, b=img, sb=st, dtype=0, mask=None, mode=PLAIN, B=1, H=4, W=4, out0=out[0], out1=out[1]):
        _lib.call("ps_percsim_input", a, sa, b, sb, dtype, mask, mode, B, H, W, out0, out1)

    negative = (ctypes.c_int64 * 4)(48, 16, -4, 1)
    refusals = [
        (tap, dict(H=64), "multiples of 128"), (tap, dict(H=200), "multiples of 128"), (tap, dict(W=192), "multiples of 128"),
        (tap, dict(H=0), "multiples of 128"), (tap, dict(C=96), "C a multiple of 64"), (tap, dict(C=0), "C a multiple of 64"),
        (tap, dict(layer=5), "layer 5"), (tap, dict(layer=-1), "layer -1"),
        (tap, dict(P=0), "1 <= P <= 65535"), (tap, dict(P=65536), "1 <= P <= 65535"),
        (tap, dict(nbytes=need - 1), "workspace of %d bytes required" % need),
        (tap, dict(y=odd[1:]), "16-byte aligned"), (tap, dict(pooled=odd[1:]), "16-byte aligned"),
        (tap, dict(y=None), "null pointer"), (tap, dict(ws=None), "null pointer"),
        (finish, dict(P=0), "1 <= P <= 65535"), (finish, dict(P=65536), "1 <= P <= 65535"),
        (finish, dict(H=64), "multiples of 128"), (finish, dict(W=200), "multiples of 128"),
        (finish, dict(nbytes=need - 1), "workspace of %d bytes required" % need),
        (finish, dict(ws=None), "null pointer"), (finish, dict(layers=None), "null pointer"), (finish, dict(total=None), "null pointer"),
        (inp, dict(mask=mask), "a mask goes with"), (inp, dict(mode=VIS), "a mask goes with"), (inp, dict(mode=INVIS), "a mask goes with"),
        (inp, dict(mode=RAW, mask=mask), "PS_PERCSIM_RAW takes fp32 images and no mask"),
        (inp, dict(mode=RAW, a=img8, b=img8, dtype=1), "PS_PERCSIM_RAW takes fp32 images and no mask"),
        (inp, dict(sa=negative), "negative stride"), (inp, dict(sb=negative), "negative stride"),
        (inp, dict(mode=4), "mode 4"), (inp, dict(mode=-1), "mode -1"), (inp, dict(dtype=2), "dtype must be"),
        (inp, dict(B=0), "1 <= B <= 65535"), (inp, dict(B=65536), "1 <= B <= 65535"),
        (inp, dict(H=0), "H = 0"), (inp, dict(W=0), "W = 0"), (inp, dict(H=65536, W=32768), "H = 65536, W = 32768"),
        (inp, dict(out0=odd[1:]), "16-byte aligned"), (inp, dict(out1=odd[1:]), "16-byte aligned"),
        (inp, dict(b=None), "null pointer"), (inp, dict(out0=None), "null pointer"), (inp, dict(sa=None), "null pointer"),
    ]
    for fn, change, why in refusals:
        with pytest.raises(RuntimeError, match="ps_percsim_(tap|finish|input) failed.*" + why):
            fn(**change)
    torch.cuda.synchronize()
    assert bool((ws == WS_FILL).all()) and bool((odd == 1).all()), "nothing was launched"
    for buf in (pooled, layers, total, out):
        assert bool((buf == SENTINEL).all()), "nothing was launched"
    # the same calls with nothing changed run: two images of ones have a cosine of 1 at every pixel
    ws[:-1] = 0
    tap()
    finish()
    inp()
    # (64 / (8 + 1e-10)^2 is 1 - 2.5e-11: the score of layer 4 is that far from 0)
    assert bool((pooled == 1).all()) and layers[0, :4].tolist() == [1.0] * 4 and 0 <= float(layers[0, 4]) < 1e-10 and total.tolist() == [4.0]
    assert same_bits(out[0].cpu(), input_mirror(img.cpu(), None, PLAIN)[0]) and torch.equal(out[0], out[1])
