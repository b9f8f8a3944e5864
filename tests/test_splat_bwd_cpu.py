"""CPU-only: the yardstick of the splat's backward pass (tests/_splat_bwd_ref.py) is pinned before the GPU tests lean on it.

torch.autograd.gradcheck in fp64, default eps / atol / rtol, on the reference formula for every accumulation mode at tau 1 and 2 and on
the restatement of project_pts; the formula's forward against _splat_ref.composite64 and its recomputed distances against the oracle's;
the z gradient exactly 0.  gradcheck differentiates numerically, so the points are built with every hit's d2 / denom at least 1e-2 away
from both clamp bounds (asserted on the oracle's dist), and the depths with |P_z| > 10 EPS.
"""
import numpy as np
import pytest
import torch

import _splat_bwd_ref as ref
import _splat_ref as sr
from pixelsynth_amd import synthetic as syn

CASE_BY_ID = {c.id: c for c in sr.CASES}


def _tiny(acc, tau):
    """S = 8, N = 40, K = 4, r = 2.5, C = 2: points resampled (a fixed stream) until no hit is within 1e-2 of a clamp bound"""
    c = sr._case(f"gradcheck_{acc}_tau{tau:g}", 8, 40, 4, 2.5, B=1, C=2, tau=tau, acc=acc, ksize=3, seed=900)
    pts, feat = sr.build(c)
    rs = np.random.RandomState(901)
    for _ in range(200):
        o = sr.oracle(c, pts, feat)
        r = o["dist"].astype(np.float64) / sr.denom64(c.S, c.r, c.rad_pow)
        bad = (o["idx"] >= 0) & ((r < ref.D_LO + 1e-2) | (r > 1.0 - 1e-2))
        if not bad.any():
            break
        for n in np.unique(o["idx"][bad]):
            pts[0, n, :2] = (rs.rand(2) * 2 - 1) * c.spread
    assert not bad.any()
    assert (o["idx"] >= 0).sum() > 100 and (o["idx"][..., -1] >= 0).any()   # (the K cap is reached)
    return c, pts, feat, o


@pytest.mark.parametrize("tau", [1.0, 2.0])
@pytest.mark.parametrize("acc", ["alphacomposite", "wsum", "wsumnorm"])
def test_gradcheck_of_the_reference_formula(acc, tau):
    c, pts, feat, o = _tiny(acc, tau)
    p = torch.from_numpy(pts).double().requires_grad_()
    f = torch.from_numpy(feat).double().requires_grad_()
    fn = lambda p_, f_: ref.splat_formula(p_, f_, o["idx"], c.S, c.r, c.rad_pow, c.tau, c.acc)
    assert torch.autograd.gradcheck(fn, (p, f))
    out = fn(p, f)
    gp, = torch.autograd.grad(out.sum(), (p,))
    assert gp[..., :2].abs().max() > 0 and not gp[..., 2].any()


def test_gradcheck_of_the_projection_restatement():
    W, B = 8, 2
    cam = syn.mp3d_cameras(B, 75.0)
    RT2inv, RT2 = syn.yaw_pose(cam["P"], 0.3, 0.1)
    RT2[:, :3, 3] += np.array([0.2, -0.1, 0.3], np.float32)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).double()
    depth = t(syn.depth_uniform(3, B, W, 1.0, 10.0).reshape(B, 1, -1)).requires_grad_()
    args = [t(cam["K"]), t(cam["Kinv"]), t(cam["Pinv"]), t(RT2)]
    fn = lambda d: ref.project_formula(d, *args, W)
    assert float(fn(depth).detach()[:, 2].abs().min()) > 10 * ref.EPS
    assert torch.autograd.gradcheck(fn, (depth,))


@pytest.mark.parametrize("case_id", ["division_S40", "wsumnorm_tau2", "rad_pow3_C5", "sort_len_129"])
def test_the_formula_is_the_oracles_compositing(case_id):
    """In fp64 its forward is composite64 up to the fp32 rounding of the oracle's distances (<= 5e-6 x the feature scale); the
    distances it recomputes are the oracle's to 1e-6 relative"""
    c = CASE_BY_ID[case_id]
    pts, feat, o, c64, _ = sr.reference(c)
    out = ref.splat_formula(torch.tensor(pts).double(), torch.tensor(feat).double(), o["idx"], c.S, c.r, c.rad_pow, c.tau, c.acc)
    err = float(np.abs(out.numpy() - c64).max())
    print(f"{case_id}: max |formula64 - composite64| = {err:.3e}")
    assert err <= 5e-6 * c.scale
    hit = o["idx"] >= 0
    n = np.where(hit, o["idx"] % c.N, 0)
    centre = -1.0 + (2.0 * (c.S - 1 - np.arange(c.S)) + 1.0) / c.S
    b = np.arange(c.B).reshape(-1, 1, 1, 1)
    p = pts.astype(np.float64)
    d2 = (-p[b, n, 0] - centre.reshape(1, 1, -1, 1)) ** 2 + (-p[b, n, 1] - centre.reshape(1, -1, 1, 1)) ** 2
    # fp32: the centre, the point and each difference are rounded once (|values| <= spread + 1 + r), the squares and their sum once each
    u, r = 2.0 ** -24, 2.0 * c.r / c.S
    bound = 2 * r * 3 * u * (c.spread + 1 + r) + 4 * u * r * r
    err = float(np.abs(d2 - o["dist"])[hit].max())
    print(f"{case_id}: max |d2_64 - dist_oracle| = {err:.3e} ({err / r ** 2:.3e} r^2), bound {bound:.3e}")
    assert err <= bound


def test_the_new_library_is_registered():
    from pixelsynth_amd import _lib, _libraries
    entry = {e.name: e for e in _libraries.LIBRARIES}["splat_bwd"]
    assert entry.so == "libpixelsynth_splat_bwd.so" and entry.headers == ("pixelsynth_splat_bwd.h",)
    assert entry.last_error == "ps_splat_bwd_last_error" and [u for u, _ in entry.units] == ["splat_bwd.hip"]
    assert set(_lib.PROTOS["splat_bwd"]) == {"ps_splat_bwd_last_error", "ps_splat_bwd_workspace_bytes", "ps_splat_backward_f32",
                                              "ps_project_pts_backward_f32"}
    from abi_util import assert_library_matches_header
    assert_library_matches_header("splat_bwd")
    assert _lib.call("ps_splat_bwd_workspace_bytes", 2, 40, 16) >= 2 * 2 * 40 * 40 * 16 * 4
    assert _lib.call("ps_splat_bwd_workspace_bytes", 0, 40, 16) == 0


def test_host_tensors_are_refused_before_a_stream_is_touched():
    from pixelsynth_amd import _lib
    z = torch.zeros(4)
    with pytest.raises(RuntimeError, match=r"ps_splat_backward_f32: args\[0\] is a CPU tensor.*no CPU fallback"):
        _lib.call("ps_splat_backward_f32", z, z, z, z, z, 1, 1, 1, 2, 1.0, 1, 1.0, 2, 0, z, z, z, 4)
    with pytest.raises(RuntimeError, match=r"ps_project_pts_backward_f32: args\[0\] is a CPU tensor"):
        _lib.call("ps_project_pts_backward_f32", z, z, z, z, z, z, 1, 2, z)
