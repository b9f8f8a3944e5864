"""GPU: the AR plan's orders worked out on the device (ps_plan_order, csrc/ar_order.hip) against the host's ps_ar_plan on the same masks,
bit for bit -- order_loc, region, first sampled ranks, set pixels -- and build_ar_plan's device route against its host route, down to
the codes of an outpainted batch.  ps_ar_plan is itself pinned to the oracle and to the reference's recorded orders
(tests/test_order_masks.py, tests/test_host_order*.py); nothing here has a tolerance."""
import functools

import numpy as np
import pytest
import torch

from pixelsynth_amd import _lib
from pixelsynth_amd import synthetic as syn
from pixelsynth_amd.ar_plan import build_ar_plan

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = [(256, 32), (64, 32), (32, 32), (24, 8), (4, 4), (3, 1)]


def tt(a):
    return torch.from_numpy(np.array(a)).to(DEV)          # (a copy: the shared references are read-only)


def _pixels(blocks, blk):
    return np.kron(blocks.astype(np.uint8), np.ones((blk, blk), np.uint8))


def _block_bernoulli(rng, p, G, blk):
    """blocks set with probability p; a tenth of the blocks made mixed (one pixel of the block turned over)"""
    m = _pixels(rng.rand(G, G) < p, blk)
    for q in rng.permutation(G * G)[:max(1, G * G // 10)]:
        y, x = (q // G) * blk + rng.randint(blk), (q % G) * blk + rng.randint(blk)
        m[y, x] ^= 1
    return m


def _masks(S, G, seed=0):
    """name -> (S,S) uint8 mask"""
    blk, rng = S // G, np.random.RandomState(1000 * S + G + seed)
    yy, xx = np.meshgrid(np.arange(S), np.arange(S), indexing="ij")
    by, bx = np.meshgrid(np.arange(G), np.arange(G), indexing="ij")
    out = {"all_background": np.ones((S, S), np.uint8), "all_foreground": np.zeros((S, S), np.uint8)}
    mixed = np.zeros((S, S), np.uint8)           # one pixel set per block: no region, D = 0 everywhere, a pure tie-break walk
    mixed[(yy % blk == (yy // blk + 1) % blk) & (xx % blk == (xx // blk + 2) % blk)] = 1
    out["every_block_mixed"] = mixed
    out["right_half"] = (xx >= S // 2).astype(np.uint8)
    one = np.zeros((G, G), bool)
    one[(2 * G) // 3, G // 3] = True
    out["one_background_block"], out["one_foreground_block"] = _pixels(one, blk), _pixels(~one, blk)
    out["checkerboard"] = _pixels((by + bx) % 2 == 0, blk)
    out["background_frame"] = _pixels((by == 0) | (by == G - 1) | (bx == 0) | (bx == G - 1), blk)
    for p in (0.02, 0.5, 0.98):
        out[f"blocks_p{p}"] = _block_bernoulli(rng, p, G, blk)
    out["pixels_p0.999"] = ((rng.rand(S, S) < 0.999) * np.where(rng.rand(S, S) < 0.5, 255, 1)).astype(np.uint8)
    if S == 256:
        out.update({"synthetic_" + k: v.astype(np.uint8) for k, v in syn.background_masks(S).items()})
    return out


def _host(bg, G):
    """ps_ar_plan on (B,S,S) uint8 masks -> order_loc, region, first_steps (frame by frame: ps_ar_plan reports a batch's minimum), counts"""
    B, S, _ = bg.shape
    L = G * G
    order, region = np.zeros((B, L), np.int32), np.zeros((B, L), np.uint8)
    first, one = np.zeros(B, np.int32), np.zeros(1, np.int32)
    _lib.call("ps_ar_plan", bg, B, S, G, order, region, None, None, None, one)
    o1, r1 = np.zeros((1, L), np.int32), np.zeros((1, L), np.uint8)
    for b in range(B):
        _lib.call("ps_ar_plan", bg[b:b + 1], 1, S, G, o1, r1, None, None, None, first[b:b + 1])
        assert np.array_equal(o1[0], order[b]) and np.array_equal(r1[0], region[b])
    assert one[0] == first.min()
    return order, region, first, np.count_nonzero(bg.reshape(B, -1), axis=1).astype(np.int32)


@functools.lru_cache(maxsize=None)
def _pool(S, G):
    """every mask of a shape, and the host's results for them: computed once, read by every test"""
    masks = _masks(S, G)
    names, bg = list(masks), np.ascontiguousarray(np.stack(list(masks.values())))
    ref = _host(bg, G)
    for a in (bg,) + ref:
        a.setflags(write=False)
    return names, bg, ref


def _device(bg, G, first=True, counts=True):
    """ps_plan_order on device masks -> numpy order_loc, region, first_steps / None, bg_counts / None (buffers pre-filled with a mark)"""
    B, S, _ = bg.shape
    L = G * G
    order = torch.full((B, L), -7, dtype=torch.int32, device=DEV)
    region = torch.full((B, L), 9, dtype=torch.uint8, device=DEV)
    fs = torch.full((B,), -7, dtype=torch.int32, device=DEV) if first else None
    cn = torch.full((B,), -7, dtype=torch.int32, device=DEV) if counts else None
    _lib.call("ps_plan_order", bg, B, S, G, order, region, fs, cn)
    torch.cuda.synchronize()
    return tuple(None if t is None else t.cpu().numpy() for t in (order, region, fs, cn))


def _assert_equal(got, ref, rows, what):
    for g, r, field in zip(got, ref, ("order_loc", "region", "first_steps", "bg_counts")):
        assert np.array_equal(g, r[rows]), (what, field)


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("S,G", SHAPES)
def test_plan_order_is_the_hosts_ar_plan(S, G, B):
    """Every mask of the shape, alone (B = 1) and in batches of three different ones."""
    names, bg, ref = _pool(S, G)
    n = len(names)
    dbg = tt(bg)
    for i in range(0, n, B):
        rows = np.arange(i, i + B) % n
        frames = dbg[i:i + B] if i + B <= n else dbg[torch.from_numpy(rows).to(DEV)]
        got = _device(frames.contiguous(), G)
        order = got[0]
        assert np.array_equal(np.sort(order, 1), np.tile(np.arange(G * G, dtype=np.int32), (B, 1))), [names[r] for r in rows]
        _assert_equal(got, ref, rows, [names[r] for r in rows])


def test_plan_order_130_different_frames():
    """(32,32), a pixel per block: more frames than one round of workgroups per XCD holds, every frame different."""
    S = G = 32
    _, bg, _ = _pool(S, G)
    rng = np.random.RandomState(77)
    seen, frames = set(), []
    for f in list(bg) + [_block_bernoulli(rng, p, G, 1) for p in np.linspace(0.01, 0.99, 130)]:
        if f.tobytes() not in seen and len(frames) < 130:      # (at one pixel per block some masks of the pool coincide)
            seen.add(f.tobytes())
            frames.append(f)
    frames = np.ascontiguousarray(np.stack(frames))
    assert len(frames) == 130
    _assert_equal(_device(tt(frames), G), _host(frames, G), np.arange(130), "130 frames")


def test_plan_order_reads_unaligned_masks_bytewise():
    """Masks that do not start at a multiple of 16 bytes take the byte-wise pooling loop: the same results."""
    S, G = 64, 32
    names, bg, ref = _pool(S, G)
    buf = torch.zeros(bg.size + 16, dtype=torch.uint8, device=DEV)
    for off in (1, 8):
        view = buf[off:off + bg.size].view(bg.shape)
        view.copy_(tt(bg))
        assert view.data_ptr() % 16 == off
        _assert_equal(_device(view, G), ref, np.arange(len(names)), f"offset {off}")


def test_plan_order_null_outputs_leave_the_others_unchanged():
    S, G = 256, 32
    names, bg, ref = _pool(S, G)
    dbg, rows = tt(bg[:5]), np.arange(5)
    for first, counts in ((False, False), (True, False), (False, True)):
        got = _device(dbg, G, first, counts)
        assert (got[2] is None) == (not first) and (got[3] is None) == (not counts)
        for g, r, field in zip(got, ref, ("order_loc", "region", "first_steps", "bg_counts")):
            assert g is None or np.array_equal(g, r[rows]), field


@pytest.mark.parametrize("S,G", [(256, 64), (100, 32), (0, 32)])
def test_plan_order_refuses_what_takes_refuses(S, G):
    assert _lib.call("ps_plan_order_takes", S, G) == 0
    bg = torch.ones(1, max(S, 1), max(S, 1), dtype=torch.uint8, device=DEV)
    order = torch.full((1, G * G), -7, dtype=torch.int32, device=DEV)
    region = torch.full((1, G * G), 9, dtype=torch.uint8, device=DEV)
    L = _lib.library("plan")
    rc = L.ps_plan_order(bg.data_ptr(), 1, S, G, order.data_ptr(), region.data_ptr(), None, None, _lib.current_stream())
    assert rc != 0 and b"not taken" in L.ps_plan_last_error()
    with pytest.raises(RuntimeError, match=r"ps_plan_order failed \(rc=-?\d+\): plan_order: S = %d, G = %d is not taken" % (S, G)):
        _lib.call("ps_plan_order", bg, 1, S, G, order, region, None, None)
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.call("ps_plan_order", bg, 1, 32, 32, None, region, None, None)
    with pytest.raises(RuntimeError, match="B must be > 0"):
        _lib.call("ps_plan_order", bg, 0, 32, 32, order, region, None, None)
    torch.cuda.synchronize()
    assert bool((order == -7).all()) and bool((region == 9).all())     # nothing was launched


def _make_model(S=256, K=128):
    """the model of tests/test_zbuffermodel_gpu.py: synthetic PixelCNN weights, the product settings"""
    import types
    from pixelsynth_amd.z_buffermodel import ZbufferModelPts
    o = dict(W=S, use_rgb_features=True, splatter="xyblending", learn_default_feature=True, radius=4, pp_pixel=K, tau=1.0,
             rad_pow=2, accumulation="alphacomposite", background_smoothing_kernel_size=13, min_z=1.0, max_z=100.0,
             rotation=0.6, direction="R", temperature=0.7, model_setting="gen_img", seed=0, homography=False)
    m = ZbufferModelPts(types.SimpleNamespace(**o)).eval()
    m.outpaint2.load_state_dict({k: torch.from_numpy(v) for k, v in syn.pixelcnn_state_dict(0).items()})
    return m.to(DEV)


def _assert_same_plan(dev, host):
    for f in ("order_loc", "region", "mask_init", "mask_undilated", "mask_dilated"):
        assert torch.equal(getattr(dev, f), getattr(host, f)), f
    assert np.array_equal(dev.order_host, host.order_host) and dev.order_host.dtype == host.order_host.dtype
    assert np.array_equal(dev.first_steps, host.first_steps) and dev.first_steps.dtype == host.first_steps.dtype
    assert dev.first_step == host.first_step and np.array_equal(dev.n_sampled, host.n_sampled) and (dev.H, dev.W) == (host.H, host.W)
    assert (dev.first_steps_dev is None) == (host.first_steps_dev is None)
    if host.first_steps_dev is not None:
        assert torch.equal(dev.first_steps_dev, host.first_steps_dev) and dev.first_steps_dev.dtype == host.first_steps_dev.dtype
    assert (dev.waves_frames is None) == (host.waves_frames is None)
    for got, want in ((dev.waves, host.waves), (dev.waves_frames, host.waves_frames)):
        if want is not None:
            assert torch.equal(got[0].cpu(), want[0].cpu()) and np.array_equal(got[1], want[1])
    assert dev.background_counts == host.background_counts


def _five_masks():
    names, bg, _ = _pool(256, 32)
    pick = ["synthetic_right_half", "synthetic_half_plus_island", "blocks_p0.5", "synthetic_ragged", "pixels_p0.999"]
    return tt(bg[[names.index(n) for n in pick]])


@pytest.mark.parametrize("as_bool", [False, True])
def test_build_ar_plan_device_route_is_the_host_route(as_bool):
    bg = _five_masks()
    bg = (bg != 0) if as_bool else bg          # (a bool mask is handed over as the bytes it is; uint8 masks may hold any nonzero value)
    for count in (False, True):
        host = build_ar_plan(bg, 32, count_background=count, order_on="host")
        dev = build_ar_plan(bg, 32, count_background=count, order_on="device")
        assert host.waves_frames is not None and (host.background_counts is not None) == count
        _assert_same_plan(dev, host)
    with pytest.raises(ValueError, match="not a shape"):
        build_ar_plan(bg[:, :100, :100], 32, order_on="device")


def test_build_ar_plan_reads_the_route_from_the_environment(monkeypatch):
    bg = _five_masks()
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    monkeypatch.setenv("PS_PLAN_ORDER", "host")
    host = build_ar_plan(bg, 32, count_background=True)
    assert "ps_ar_plan" in calls and "ps_plan_order" not in calls
    del calls[:]
    monkeypatch.delenv("PS_PLAN_ORDER")
    build_ar_plan(bg, 32)
    assert "ps_ar_plan" in calls and "ps_plan_order" not in calls       # host is the default
    del calls[:]
    monkeypatch.setenv("PS_PLAN_ORDER", "device")
    dev = build_ar_plan(bg, 32, count_background=True)
    assert "ps_plan_order" in calls and "ps_ar_plan" not in calls
    _assert_same_plan(dev, host)


def test_outpainted_codes_do_not_depend_on_the_route(monkeypatch):
    """plan_views at 4 views under each setting of PS_PLAN_ORDER, then outpaint_planned with the same uniforms: the same codes."""
    m = _make_model()
    V = 4
    cam = syn.demo_cameras(V)
    img, depth = tt(syn.image(61, V, 3, 256)), tt(syn.depth_smooth(62, V, 256, 1.0, 100.0))
    rts = [syn.yaw_pose(cam["P"][v:v + 1], y) for v, y in enumerate((0.6, -0.3, 0.45, -0.55))]
    RT2, RT2inv = tt(np.concatenate([r[1] for r in rts])), tt(np.concatenate([r[0] for r in rts]))
    codes, uni = tt(syn.codes(63, V)), tt(np.random.RandomState(64).rand(V, 1024).astype(np.float32))
    args = (img, depth, tt(cam["K"]), tt(cam["Kinv"]), tt(cam["P"]), tt(cam["Pinv"]), RT2, RT2inv)
    out = {}
    for route in ("host", "device"):
        monkeypatch.setenv("PS_PLAN_ORDER", route)
        planned = m.plan_views(*args)
        out[route] = (planned["plan"], m.outpaint_planned(planned, codes, temperature=0.7, uniforms=uni)["codes"].clone())
        torch.cuda.synchronize()
        m.outpaint2.engine(32, 32, V).check()
    _assert_same_plan(out["device"][0], out["host"][0])
    assert torch.equal(out["device"][1], out["host"][1])
