"""GPU: the backward pass of the soft z-buffer splat and of the reprojection (csrc/splat_bwd.hip behind include/pixelsynth_splat_bwd.h,
the autograd Functions of layers/z_buffer_layers.py and projection/z_buffer_manipulator.py).

One bar for every gradient (tests/_splat_bwd_ref.py states it and why): g64 = fp64 autograd of the reference formula on the CPU, g32 the
same formula in fp32, E32 = max |g32 - g64|, and max |g_hip - g64| <= 4 max(E32, 1e-6 max |g64|).  The points with a hit within 1e-4 of a
clamp bound (by the oracle's dist) can fall on either side of the kink in fp32 and fp64: they are left out of the grad_pts comparison
alone (at most 2 % of the points that have a hit), and E32 is taken over the points that are compared.  The largest ratio
max |g_hip - g64| / E32 of every case is printed.

At tau < 1 the accuracy of grad_pts is NOT pinned (the derivative of alpha is unbounded at the rim of a disc; the fp32 formula itself is
only within 1e-4 of fp64 there): tau0.5_S40 asserts grad_feat at the bar and grad_pts finite everywhere.
"""
import types

import numpy as np
import pytest
import torch

import _splat_bwd_ref as ref
import _splat_ref as sr
from oracle import c_oracle
from pixelsynth_amd import _lib, synthetic as syn

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CASE_BY_ID = {c.id: c for c in sr.CASES}
CASE_IDS = ref.OPERATOR_CASE_IDS
_REF = {}


def _splatter(c):
    from pixelsynth_amd.layers.z_buffer_layers import RasterizePointsXYsBlending
    opts = types.SimpleNamespace(tau=c.tau, rad_pow=c.rad_pow, accumulation=c.acc, background_smoothing_kernel_size=c.ksize)
    return RasterizePointsXYsBlending(c.C, learn_feature=False, radius=c.r, size=c.S, points_per_pixel=c.K, opts=opts)


def _reference(c):
    """(pts, feat, oracle, grad_out, (out, grad_pts, grad_feat) in fp64, the same in fp32) of a case: once per process, read-only"""
    if c.id not in _REF:
        pts, feat, o, _, _ = sr.reference(c)
        g = np.random.RandomState(c.seed + 7000).randn(c.B, c.C, c.S, c.S).astype(np.float32)
        _REF[c.id] = (pts, feat, o, g, ref.case_gradients(c, pts, feat, o["idx"], g, torch.float64),
                      ref.case_gradients(c, pts, feat, o["idx"], g, torch.float32))
    return _REF[c.id]


def _hip(c, pts, feat, g, want_pts=True, want_feat=True):
    """Through the module on the device -> (features, mask, grad_pts or None, grad_feat or None, the caller's points after the call)"""
    p = torch.tensor(pts, device=DEV).requires_grad_(want_pts)
    f = torch.tensor(feat, device=DEV).requires_grad_(want_feat)
    out, bg = _splatter(c)(p, f)
    assert out.requires_grad and out.grad_fn is not None and not bg.requires_grad and bg.dtype == torch.bool
    out.backward(torch.tensor(g, device=DEV))
    torch.cuda.synchronize()
    return out.detach(), bg, p.grad, f.grad, p.detach()


def _at_the_bar(name, got, g64, g32, keep=None):
    got = got.detach().cpu().double().numpy()
    if keep is not None:
        got, g64, g32 = got[keep], g64[keep], g32[keep]
    bound, e32 = ref.bar(g64, g32)
    err = float(np.abs(got - g64).max())
    scale = float(np.abs(g64).max())
    print(f"{name}: max |hip - g64| = {err:.3e}, E32 = {e32:.3e} ({e32 / scale:.2e} max |g64|), ratio {err / max(e32, 1e-300):.3f}, "
          f"bound {bound:.3e}")
    assert scale > 0 and err <= bound, (name, err, bound)


def check_gradients(c):
    """A case through the module against the fp64 autograd of the formula: the forward's bits against the debug route, exact zeros for
    unseen points and for z, both gradients at the bar -> (grad_pts, grad_feat, the debug route's idx and dist) on the device.  Shared with
    tests/test_train_routes2_gpu.py, whose cases are not in _splat_ref.CASES."""
    pts, feat, o, g, (_, gp64, gf64), (_, gp32, gf32) = _reference(c)
    out, bg, gp, gf, after = _hip(c, pts, feat, g)
    assert gp.shape == (c.B, c.N, 3) and gf.shape == (c.B, c.C, c.N) and gp.dtype == gf.dtype == torch.float32
    assert torch.equal(after.cpu(), torch.from_numpy(np.array(pts))), "the differentiable route must leave the caller's points alone"
    # forward: the bits of return_debug=True's features, the plain route's mask
    with torch.no_grad():
        dbg = _splatter(c)(torch.tensor(pts, device=DEV), torch.tensor(feat, device=DEV), return_debug=True)
        plain = _splatter(c)(torch.tensor(pts, device=DEV), torch.tensor(feat, device=DEV))
    assert torch.equal(out, dbg[0]) and torch.equal(bg, plain[1]) and np.array_equal(bg.cpu().numpy(), o["bg"])
    assert np.array_equal(dbg[2].cpu().numpy(), o["idx"])
    # points in no list: exact zeros; z: exact zeros
    seen = ref.hit_points(o["idx"], c.B, c.N)
    assert seen.any() and ((~seen).any() or c.id == "sort_len_129")     # (the pile: every point is on the one pixel's list)
    gpn, gfn = gp.cpu().numpy(), gf.cpu().numpy()
    assert not gpn[..., 2].any()
    assert not gpn[~seen].any() and not gfn.transpose(0, 2, 1)[~seen].any()
    _at_the_bar(f"{c.id} grad_feat", gf, gf64, gf32)
    if c.tau < 1.0:
        assert np.isfinite(gpn).all()      # (accuracy of grad_pts not pinned at tau < 1: see the module docstring)
        return gp, gf, dbg[2], dbg[4]
    kink = ref.kink_points(c, o["idx"], o["dist"], c.B, c.N)
    print(f"{c.id}: {kink.sum()} of {seen.sum()} points with a hit lie within {ref.KINK:g} of a clamp bound")
    assert kink.sum() <= 0.02 * seen.sum()
    _at_the_bar(f"{c.id} grad_pts", gp[..., :2], gp64[..., :2], gp32[..., :2], keep=~kink)
    return gp, gf, dbg[2], dbg[4]


@pytest.mark.parametrize("case_id", CASE_IDS)
def test_gradients_against_fp64_autograd(case_id):
    check_gradients(CASE_BY_ID[case_id])


def test_two_runs_and_a_cloud_alone_give_the_same_bits():
    c = CASE_BY_ID["division_S40"]
    pts, feat, o, g, _, _ = _reference(c)
    first, again = _hip(c, pts, feat, g), _hip(c, pts, feat, g)
    for name, p, q in zip(("features", "mask", "grad_pts", "grad_feat"), first, again):
        assert torch.equal(p, q), name
    for b in range(c.B):
        alone = _hip(c._replace(B=1), pts[b:b + 1], feat[b:b + 1], g[b:b + 1])
        for name, p, q in zip(("features", "mask", "grad_pts", "grad_feat"), first, alone):
            assert torch.equal(p[b:b + 1], q), (name, b)


@pytest.mark.parametrize("which", ["pts", "src"])
def test_only_the_gradient_asked_for(which):
    c = CASE_BY_ID["division_S40"]
    pts, feat, o, g, _, _ = _reference(c)
    both = _hip(c, pts, feat, g)
    one = _hip(c, pts, feat, g, want_pts=which == "pts", want_feat=which == "src")
    assert (one[2] is None) == (which == "src") and (one[3] is None) == (which == "pts")
    k = 2 if which == "pts" else 3
    assert torch.equal(one[k], both[k]) and torch.equal(one[0], both[0])


def test_no_grad_takes_the_plain_route(monkeypatch):
    """Nothing requires grad, or grad mode is off: the route of always -- the caller's points negated in place, no saved lists"""
    c = CASE_BY_ID["division_S40"]
    pts, feat, o, g, _, _ = _reference(c)
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    p, f = torch.tensor(pts, device=DEV), torch.tensor(feat, device=DEV)
    out, bg = _splatter(c)(p, f)
    assert out.grad_fn is None and np.array_equal(p.cpu().numpy(), o["pts_after"])
    p2 = torch.tensor(pts, device=DEV)
    with torch.no_grad():
        out2, _ = _splatter(c)(p2, torch.tensor(feat, device=DEV).requires_grad_())
    assert out2.grad_fn is None and torch.equal(out, out2) and torch.equal(p, p2)
    assert "ps_splat_backward_f32" not in calls and calls.count("ps_splat_f32") == 2


# ------------------------------------------------------------------------------------------------------------------ projection
def _cameras(B, seed):
    """Random intrinsics (a field of view) and poses (yaw, pitch, a translation) on pixelsynth_amd.synthetic's constructions"""
    rs = np.random.RandomState(seed)
    cam = syn.mp3d_cameras(B, float(rs.uniform(60.0, 100.0)))
    RT2 = np.concatenate([syn.yaw_pose(cam["P"][b:b + 1], float(rs.uniform(-0.3, 0.3)), float(rs.uniform(-0.15, 0.15)))[1] for b in range(B)])
    RT2[:, :3, 3] += rs.uniform(-0.2, 0.2, (B, 3)).astype(np.float32)
    return [np.ascontiguousarray(a, np.float32) for a in (cam["K"], cam["Kinv"], cam["P"], cam["Pinv"], RT2, np.linalg.inv(RT2))]


def _manipulator(W, C=3, radius=2.0, K=8, tau=1.0, acc="alphacomposite"):
    from pixelsynth_amd.projection.z_buffer_manipulator import PtsManipulator
    opt = types.SimpleNamespace(splatter="xyblending", learn_default_feature=False, radius=radius, pp_pixel=K, tau=tau, rad_pow=2,
                                accumulation=acc, background_smoothing_kernel_size=3)
    return PtsManipulator(W, C=C, opt=opt).to(DEV)


def _project_gradients(depth, cams, W, g, dtype):
    K, Kinv, P, Pinv, RT2, RT2inv = [torch.from_numpy(a).to(dtype) for a in cams]
    d = torch.from_numpy(depth).to(dtype).requires_grad_()
    s = ref.project_formula(d, K, Kinv, Pinv, RT2, W)
    return s.detach().double().numpy(), torch.autograd.grad(s, d, torch.from_numpy(g).to(dtype))[0].double().numpy()


@pytest.mark.parametrize("degenerate", [False, True])
def test_project_pts_backward(degenerate):
    W, B = 16, 2
    cams = _cameras(B, 11)
    depth = syn.depth_uniform(12, B, W, 1.0, 10.0).reshape(B, 1, W * W)
    if degenerate:      # depths at which the projected z is inside EPS, chosen on the restatement (P_z is affine in the depth: two
        # evaluations give its root): the sampler is the constant -10 there
        K, Kinv, P, Pinv, RT2, RT2inv = [torch.from_numpy(a).double() for a in cams]
        z1, z2 = [-ref.project_formula(torch.full((B, 1, W * W), v, dtype=torch.float64), K, Kinv, Pinv, RT2, W)[:, 2].numpy() for v in (1.0, 2.0)]
        root = -(z1 - (z2 - z1)) / (z2 - z1)
        for b, n in ((0, 3), (0, 77), (0, 200), (1, 130)):
            depth[b, 0, n] = root[b, n]
    g = np.random.RandomState(13).randn(B, 3, W * W).astype(np.float32)
    s64, g64 = _project_gradients(depth, cams, W, g, torch.float64)
    _, g32 = _project_gradients(depth, cams, W, g, torch.float32)
    const = (np.abs(s64) == 10.0).all(1)          # (-10, then the sign flips of y and z)
    assert const.sum() == (4 if degenerate else 0)
    pm = _manipulator(W)
    d = torch.tensor(depth, device=DEV).requires_grad_()
    s = pm.project_pts(d, *[torch.tensor(a, device=DEV) for a in cams])
    assert s.grad_fn is not None
    with torch.no_grad():
        assert torch.equal(s, pm.project_pts(d, *[torch.tensor(a, device=DEV) for a in cams]))
    s.backward(torch.tensor(g, device=DEV))
    assert d.grad.shape == d.shape
    assert not d.grad.cpu().numpy()[:, 0][const].any() and not g64[:, 0][const].any()
    _at_the_bar(f"project_pts grad_depth (degenerate={degenerate})", d.grad, g64, g32)


# ------------------------------------------------------------------------------------------------------------------ forward_justpts
def _smooth_image(B, C, W, seed):
    rs = np.random.RandomState(seed)
    yy, xx = np.meshgrid(np.arange(W) / W, np.arange(W) / W, indexing="ij")
    img = np.empty((B, C, W, W), np.float32)
    for b in range(B):
        for ch in range(C):
            fx, fy, ph = rs.uniform(0.5, 2.0), rs.uniform(0.5, 2.0), rs.uniform(0, 6.28)
            img[b, ch] = np.sin(6.28 * (fx * xx + fy * yy) + ph)
    return img


def test_forward_justpts_end_to_end(monkeypatch):
    W, B, C, R, KP = 32, 2, 3, 2.0, 8
    cams = _cameras(B, 21)
    dcams = [torch.tensor(a, device=DEV) for a in cams]
    src = syn.image(22, B, C, W)
    depth = syn.depth_smooth(23, B, W, 2.0, 6.0)
    g = np.random.RandomState(24).randn(B, C, W, W).astype(np.float32)
    pm = _manipulator(W, C, R, KP)
    # no input requires grad: today's fused route, bit for bit, and the backward entry point is never called
    calls = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a, **k: (calls.append(name), real(name, *a, **k))[1])
    plain, plain_bg = pm.forward_justpts(torch.tensor(src, device=DEV), torch.tensor(depth, device=DEV), *dcams)
    assert plain.grad_fn is None and calls == ["ps_splat_workspace_bytes", "ps_project_splat_f32"]
    from pixelsynth_amd.layers.z_buffer_layers import splat_workspace
    fused = torch.empty(B, C, W, W, device=DEV)
    fused_bg = torch.empty(B, W, W, dtype=torch.uint8, device=DEV)
    ws = splat_workspace(torch.device(DEV), B, W * W, W, R)
    real("ps_project_splat_f32", torch.tensor(depth, device=DEV), torch.tensor(src, device=DEV), dcams[0], dcams[1], dcams[3], dcams[4], B, C, W,
         R, KP, 1.0, 2, 0, 3, fused, fused_bg, ws, ws.numel())
    assert torch.equal(plain, fused) and torch.equal(plain_bg, fused_bg.view(torch.bool))
    # under autograd
    s_dev = torch.tensor(src, device=DEV).requires_grad_()
    d_dev = torch.tensor(depth, device=DEV).requires_grad_()
    out, bg = pm.forward_justpts(s_dev, d_dev, *dcams)
    assert out.grad_fn is not None and torch.equal(bg, plain_bg)
    out.backward(torch.tensor(g, device=DEV))
    assert "ps_splat_backward_f32" in calls and "ps_project_pts_backward_f32" in calls
    # the fp64 chain: the restatement of the projection, then the formula on the oracle's lists for the fp32 projected points
    sampler32 = c_oracle.project_pts(depth.reshape(B, 1, -1), cams[0], cams[1], cams[3], cams[4], W)
    o = c_oracle.splat_forward(np.ascontiguousarray(sampler32.transpose(0, 2, 1)), src.reshape(B, C, -1), W, radius_px=R, K=KP, bg_ksize=3)

    def chain(dtype):
        K, Kinv, P, Pinv, RT2, RT2inv = [torch.from_numpy(a).to(dtype) for a in cams]
        d = torch.from_numpy(depth.reshape(B, 1, -1)).to(dtype).requires_grad_()
        f = torch.from_numpy(src.reshape(B, C, -1)).to(dtype).requires_grad_()
        pts = ref.project_formula(d, K, Kinv, Pinv, RT2, W).permute(0, 2, 1)
        res = ref.splat_formula(pts, f, o["idx"], W, R, 2, 1.0, "alphacomposite")
        gd, gf = torch.autograd.grad(res, (d, f), torch.from_numpy(g).to(dtype))
        return res.detach().double().numpy(), gd.double().numpy().reshape(B, -1), gf.double().numpy()

    (o64, gd64, gf64), (_, gd32, gf32) = chain(torch.float64), chain(torch.float32)
    assert float(np.abs(out.detach().cpu().numpy() - o64).max()) <= 1e-4
    c = sr._case("e2e", W, W * W, KP, R, B=B, C=C)
    seen, kink = ref.hit_points(o["idx"], B, W * W), ref.kink_points(c, o["idx"], o["dist"], B, W * W)
    print(f"forward_justpts: {kink.sum()} of {seen.sum()} points with a hit lie within {ref.KINK:g} of a clamp bound")
    assert seen.sum() > 0.5 * B * W * W and kink.sum() <= 0.02 * seen.sum()
    _at_the_bar("forward_justpts grad_src", s_dev.grad.reshape(B, C, -1), gf64, gf32)
    _at_the_bar("forward_justpts grad_pred_pts", d_dev.grad.reshape(B, -1), gd64, gd32, keep=~kink)
    assert d_dev.grad.shape == d_dev.shape and not d_dev.grad.reshape(B, -1).cpu().numpy()[~seen].any()


def test_depth_can_be_fitted_through_the_renderer():
    """The target is the render of depth D*; from 1.15 D*, 30 Adam steps on the depth alone under the photometric L1 of the two renders.
    Only the strict decrease of the loss is asserted."""
    W, B, C = 32, 1, 3
    cams = _cameras(B, 31)
    dcams = [torch.tensor(a, device=DEV) for a in cams]
    src = torch.tensor(_smooth_image(B, C, W, 32), device=DEV)
    d_star = torch.tensor(syn.depth_smooth(33, B, W, 2.0, 4.0), device=DEV)
    pm = _manipulator(W, C, 2.0, 8)
    with torch.no_grad():
        target, _ = pm.forward_justpts(src, d_star, *dcams)
    depth = (1.15 * d_star).clone().requires_grad_()
    before = float((depth.detach() - d_star).abs().mean())
    opt = torch.optim.Adam([depth], lr=0.02)
    losses = []
    for _ in range(30):
        opt.zero_grad()
        out, _ = pm.forward_justpts(src, depth, *dcams)
        loss = (out - target).abs().mean()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    with torch.no_grad():
        final = float((pm.forward_justpts(src, depth, *dcams)[0] - target).abs().mean())
    after = float((depth.detach() - d_star).abs().mean())
    print(f"photometric L1: {losses[0]:.5f} at the start, {final:.5f} after 30 Adam steps; mean |D - D*|: {before:.4f} before, {after:.4f} after")
    assert np.isfinite(losses).all() and final < losses[0]


# ------------------------------------------------------------------------------------------------------------------ ABI
def test_the_entry_point_refuses_what_it_cannot_do():
    B, N, C, S, K = 1, 50, 3, 16, 4
    z = lambda *s, dt=torch.float32: torch.zeros(*s, dtype=dt, device=DEV)
    pts, feat, idx, dist, g = z(B, N, 3), z(B, C, N), z(B, S, S, K, dt=torch.int32) - 1, z(B, S, S, K), z(B, C, S, S)
    gp, gf = z(B, N, 3), z(B, C, N)
    need = _lib.call("ps_splat_bwd_workspace_bytes", B, S, K)
    ws = torch.empty(need, dtype=torch.uint8, device=DEV)
    args = (pts, feat, idx, dist, g, B, N, C, S, 2.0, K, 1.0, 2, 0)
    with pytest.raises(RuntimeError, match=r"ps_splat_backward_f32 failed .*grad_pts and grad_feat are both NULL"):
        _lib.call("ps_splat_backward_f32", *args, None, None, ws, need)
    with pytest.raises(RuntimeError, match=r"ps_splat_backward_f32 failed .*workspace %d < required %d" % (need - 1, need)):
        _lib.call("ps_splat_backward_f32", *args, gp, gf, ws, need - 1)
    gp.fill_(1.0), gf.fill_(1.0)
    _lib.call("ps_splat_backward_f32", *args, gp, gf, ws, need)          # no hit anywhere: every element written, exact zeros
    torch.cuda.synchronize()
    assert not gp.any() and not gf.any()
