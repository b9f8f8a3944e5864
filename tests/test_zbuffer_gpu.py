"""GPU tests of the hard z-buffer: the z-test scatter kernel bit-exact against the sequential definition, the
DepthManipulator mirror against the reference's own outputs (tests/golden/zbuffer.npz); the projection kernel and the scatter through
a sort order, each called on its own and end to end, bit for bit against the sequential float32 mirror of tests/_zbuffer_ref.py."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

import _zbuffer_ref as zr

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
from oracle import zbuffer_oracle as zo  # noqa: E402
from pixelsynth_amd import _lib  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def test_zbuffer_scatter_kernel_is_the_sequential_last_write():
    """ps_zbuffer_scatter_f32 against numpy's in-order assignment (last write to a pixel stays) on heavy pile-ups."""
    rs = np.random.RandomState(0)
    B, N, H, W = 3, 50000, 64, 48
    ys = rs.randint(0, H, size=(B, N)).astype(np.int32)
    xs = (rs.randint(0, W, size=(B, N)) // 3 * 3 % W).astype(np.int32)      # many points per pixel, some pixels never hit
    v0, v1 = rs.randn(B, N).astype(np.float32), rs.randn(B, N).astype(np.float32)
    want = np.full((B, 2, H, W), -2.0, np.float32)
    for b in range(B):
        want[b, 0, ys[b], xs[b]] = v0[b]
        want[b, 1, ys[b], xs[b]] = v1[b]
    out = torch.full((B, 2, H, W), -2.0, device=DEV)
    winner = torch.empty(B, H, W, dtype=torch.int32, device=DEV)
    dev = [tt(a) for a in (ys, xs, v0, v1)]     # (kept alive: a temporary's block would be handed to the next upload)
    rc = _lib.lib().ps_zbuffer_scatter_f32(*[_lib.ptr(a) for a in dev], B, N, H, W, _lib.ptr(out), _lib.ptr(winner),
                                           _lib.ptr(_lib.status_word(DEV)), _lib.current_stream())
    _lib.check(rc, "ps_zbuffer_scatter_f32")
    _lib.read_status("ps_zbuffer_scatter_f32", DEV)      # synchronises; nothing was dropped
    assert np.array_equal(out.cpu().numpy(), want)
    assert (want == -2).any() and (want != -2).any()


def bits(a):
    """float32 as its int32 bits: -0.0 is not 0.0 and a NaN is its payload"""
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def gpu_project(depth, grid, K, Kinv, RT1inv, RT2, W):
    """ps_zbuffer_project_f32 on numpy inputs -> numpy (zproj, ys, xs, flag).  The outputs are prefilled, so an entry not written
    shows, and each is the head of a longer buffer whose tail must come back untouched: the workgroup of 256 that holds point N - 1
    has threads beyond it, and what they would write for the last frame lands there."""
    B, N = depth.shape
    assert N == W * W and grid.shape == (4, N)
    dev = [tt(a.astype(np.float32)) for a in (depth, grid, K, Kinv, RT1inv, RT2)]
    bufs = [torch.full((B * N + 256,), -77, dtype=dt, device=DEV) for dt in (torch.float32, torch.int32, torch.int32, torch.float32)]
    _lib.call("ps_zbuffer_project_f32", *dev, B, W, *bufs)
    bufs = [a.cpu().numpy() for a in bufs]
    assert all((a[B * N:] == -77).all() for a in bufs), "written beyond the last point of the last frame"
    return tuple(a[:B * N].reshape(B, N) for a in bufs)


def assert_projection_equal(got, want, what):
    for name, g, w in zip(("zproj", "ys", "xs", "flag"), got, want):
        g, w = (bits(g), bits(w)) if g.dtype == np.float32 else (g, w)
        assert g.dtype == w.dtype and np.array_equal(g, w), \
            f"{what}: {name} differs at {np.argwhere(g != w)[:8].tolist()}: kernel {g[g != w][:8]}, mirror {w[g != w][:8]}"


def random_projection_case():
    """W = 17: N = 289 is two workgroups of k_zb_project, the second with 33 live threads.  B = 3, every frame with cameras of its
    own: a Matterport-shaped K of another field of view, a source pose that is no identity, yaw / pitch target poses, frame 2
    looking backwards.  A random grid (its third row is not -1, its rows are not the manipulator's) and depths of both ranges of the fixture."""
    from pixelsynth_amd import synthetic as syn
    rs = np.random.RandomState(11)
    W, B = 17, 3
    N = W * W
    cams = [syn.mp3d_cameras(1, hfov) for hfov in (90.0, 70.0, 110.0)]
    K, Kinv = np.concatenate([c["K"] for c in cams]), np.concatenate([c["Kinv"] for c in cams])
    P = syn.demo_cameras(1)["P"]
    RT1inv = np.concatenate([syn.yaw_pose(P, yaw, pitch=pitch)[0] for yaw, pitch in ((0.1, 0.0), (-0.2, 0.05), (0.0, -0.1))])
    RT2 = np.concatenate([syn.yaw_pose(P, yaw, pitch=pitch)[1] for yaw, pitch in ((0.4, 0.1), (-0.6, 0.0), (3.0, 0.2))])
    grid = rs.uniform(-1.2, 1.2, size=(4, N)).astype(np.float32)
    grid[2] = rs.uniform(-1.3, -0.7, size=N)
    depth = np.where(rs.rand(B, N) < 0.5, rs.uniform(1.0, 100.0, (B, N)), rs.uniform(0.001, 0.02, (B, N))).astype(np.float32)
    return W, depth, grid, K, Kinv, RT1inv, RT2


def test_zbuffer_project_kernel_is_the_mirror_bit_for_bit():
    """ps_zbuffer_project_f32 against tests/_zbuffer_ref.py's project() on random points: every output equal, bit for bit."""
    W, depth, grid, K, Kinv, RT1inv, RT2 = random_projection_case()
    zproj, ys, xs, flag = want = zr.project(depth, grid, K, Kinv, RT1inv, RT2)
    # the case is not hollow: in range and out of range, the EPS branch, and the clamp at both ends of both axes
    bad = np.abs(zproj) < zr.EPS
    assert (flag == 0).sum() > 50 and (flag == 4).sum() > 50 and bad.sum() > 10 and (~bad).sum() > 50
    assert all((a[~bad] == v).any() for a in (xs, ys) for v in (0, 255)) and ((xs > 0) & (xs < 255) & (ys > 0) & (ys < 255)).sum() > 50
    assert all(((flag[b] == 0).any() and (flag[b] == 4).any()) for b in range(3)) and not np.array_equal(zproj[0], zproj[1])
    assert_projection_equal(gpu_project(depth, grid, K, Kinv, RT1inv, RT2, W), want, "random points")


def test_zbuffer_project_refuses_what_the_abi_refuses():
    W, depth, grid, K, Kinv, RT1inv, RT2 = random_projection_case()
    dev = [tt(a) for a in (depth, grid, K, Kinv, RT1inv, RT2)]
    outs = [torch.empty(3, W * W, device=DEV), torch.empty(3, W * W, dtype=torch.int32, device=DEV),
            torch.empty(3, W * W, dtype=torch.int32, device=DEV), torch.empty(3, W * W, device=DEV)]
    fn, stream = _lib.lib().ps_zbuffer_project_f32, _lib.current_stream()
    ptrs = [_lib.ptr(a) for a in dev + outs]
    assert fn(*ptrs[:6], 3, 1, *ptrs[6:], stream) != 0            # W = 1
    assert fn(*ptrs[:6], 0, W, *ptrs[6:], stream) != 0            # B = 0
    for i in range(len(ptrs)):
        a = ptrs[:i] + [None] + ptrs[i + 1:]
        assert fn(*a[:6], 3, W, *a[6:], stream) != 0, f"null pointer in place {i}"
    with pytest.raises(RuntimeError, match="null pointer"):
        _lib.check(fn(None, *ptrs[1:6], 3, W, *ptrs[6:], stream), "ps_zbuffer_project_f32")
    _lib.check(fn(*ptrs[:6], 3, W, *ptrs[6:], stream), "ps_zbuffer_project_f32")          # and the same call with nothing wrong
    torch.cuda.synchronize()


def test_zbuffer_project_kernel_at_its_edges():
    """The table of single points of tests/_zbuffer_ref.py: t exactly at, below and above 0 and 255 on both axes, |X[2]| around
    EPS, signed zeros, depths that are no depth.  Every row of both frames against the mirror; frame 1 (identity cameras) also
    against the literal (xs, ys, flag) written in the table, so that an error mirror and kernel share still shows."""
    case = zr.edge_case()
    args = [case[k] for k in ("depth", "grid", "K", "Kinv", "RT1inv", "RT2")]
    want = zr.project(*args)
    zproj, ys, xs, flag = got = gpu_project(*args, case["W"])
    for i, (name, _, _, g2, d, lit) in enumerate(case["rows"]):
        assert (int(xs[1, i]), int(ys[1, i]), float(flag[1, i])) == lit, f"{name}: kernel ({xs[1, i]}, {ys[1, i]}, {flag[1, i]}), expected {lit}"
        if not np.isinf(d):          # X[2] = g2 d through the identity, untouched by the EPS rule, sign of zero included
            assert bits(zproj[1, i]) == bits(np.float32(g2) * np.float32(d)), name
    assert_projection_equal(got, want, "edge table")


def pileup_case():
    """B = 2, N = 5000 points on 16 x 12 pixels, of which every third column is never hit: about 39 points per hit pixel.
    An independent random permutation per frame as the sort order, a random grid, and a flag that is random BY POSITION, so
    that flag[n] and flag[order[n]] are different numbers."""
    rs = np.random.RandomState(5)
    B, N, H, W = 2, 5000, 16, 12
    order = np.stack([rs.permutation(N) for _ in range(B)]).astype(np.int64)
    ys = rs.randint(0, H, size=(B, N)).astype(np.int32)
    xs = (rs.randint(0, W // 3 * 2, size=(B, N)) * 3 // 2).astype(np.int32)          # 0 1 3 4 6 7 9 10
    grid = rs.randn(4, N).astype(np.float32)
    flag = (rs.randint(0, 2, size=(B, N)) * 4).astype(np.float32)
    return B, N, H, W, order, ys, xs, grid, flag


def gpu_scatter_sorted(order, ys, xs, grid, flag, H, W, winner=None):
    B, N = order.shape
    out = torch.full((B, 2, H, W), 7.0, device=DEV)
    if winner is None:
        winner = torch.full((B, H, W), 0x7fffffff, dtype=torch.int32, device=DEV)
    dev = [tt(a) for a in (order, ys, xs, grid, flag)]
    _lib.call("ps_zbuffer_scatter_sorted_f32", *dev, B, N, H, W, out, winner, _lib.status_word(DEV))
    return out, winner


def test_zbuffer_scatter_sorted_kernel_is_the_mirror_on_pile_ups():
    """ps_zbuffer_scatter_sorted_f32 against scatter_sorted: the last sorted position on a pixel stays, its values are built from
    the point's grid entry and the POSITION's flag, pixels nobody hits keep the caller's 7.0, and a winner buffer full of
    0x7fffffff from the caller does not outlive the reset."""
    B, N, H, W, order, ys, xs, grid, flag = pileup_case()
    want = np.full((B, 2, H, W), 7.0, np.float32)
    assert not zr.scatter_sorted(order, ys, xs, grid, flag, H, W, want)
    assert (want[:, :, :, 2::3] == 7).all() and (want[:, :, :, 0::3] != 7).all() and (want[:, :, :, 1::3] != 7).all()
    by_point = np.full_like(want, 7.0)           # the mistake the random flag is there for
    zr.scatter_sorted(order, ys, xs, grid, np.take_along_axis(flag, order, 1), H, W, by_point)
    assert (by_point != want).mean() > 0.2
    out, winner = gpu_scatter_sorted(order, ys, xs, grid, flag, H, W)
    _lib.read_status("ps_zbuffer_scatter_sorted_f32", DEV)          # synchronises; nothing was dropped
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))
    again, _ = gpu_scatter_sorted(order, ys, xs, grid, flag, H, W, winner=winner)      # (the first run's winners: reset again)
    _lib.read_status("ps_zbuffer_scatter_sorted_f32", DEV)
    assert np.array_equal(bits(again.cpu().numpy()), bits(want))


def test_zbuffer_scatter_sorted_kernel_drops_what_the_mirror_skips():
    """The pile-ups with positions that must be dropped: order entries outside [0, N) -- among them 2^32 and 2^32 + N - 1, which are
    valid points once truncated to 32 bits, at the last sorted positions, where as points they would win -- and points whose pixel
    is outside the image.  Two of the dropped positions were the last of their pixel, so the position before them has to win."""
    B, N, H, W, order, ys, xs, grid, flag = pileup_case()
    last, count = np.full((B, H, W), -1), np.zeros((B, H, W), int)      # per pixel, before anything is dropped: the winner, the points
    for b in range(B):
        last[b, ys[b, order[b]], xs[b, order[b]]] = np.arange(N)
        np.add.at(count[b], (ys[b], xs[b]), 1)
    n_won, m_won = int(last[0, 3, 4]), int(last[1, 9, 7])
    assert count[0, 3, 4] >= 2 and count[1, 9, 7] >= 2 and n_won >= 0 and m_won >= 0
    assert len({17, 1234, N - 1, N - 2, n_won, 40, 42}) == 7 and len({2500, N - 1, m_won, 41}) == 4      # no two of the positions below coincide
    # a) entries that are no point: at scattered positions, at frame 0's last two, and at the winner of frame 0's pixel (3, 4)
    for b, n, entry in ((0, 17, -1), (1, 2500, N), (0, 1234, N + 2 ** 32), (0, N - 1, 2 ** 32), (0, N - 2, 2 ** 32 + N - 1),
                        (1, N - 1, -2 ** 31 - 5), (0, n_won, N)):
        order[b, n] = entry
    # b) points outside the image, reached through valid entries; the last of them is the winner of frame 1's pixel (9, 7)
    ys[0, order[0, 40]], ys[1, order[1, 41]], xs[0, order[0, 42]], ys[1, order[1, m_won]] = -1, H, W, H
    want, clean = np.full((B, 2, H, W), 7.0, np.float32), np.full((B, 2, H, W), 7.0, np.float32)
    assert zr.scatter_sorted(order, ys, xs, grid, flag, H, W, want)
    trunc = (order & 0xffffffff).astype(np.int64)                      # the mistake the 2^32 entries are there for
    zr.scatter_sorted(np.where(trunc < N, trunc, -1), ys, xs, grid, flag, H, W, clean)
    assert not np.array_equal(clean, want)
    out, _ = gpu_scatter_sorted(order, ys, xs, grid, flag, H, W)
    with pytest.raises(RuntimeError, match="outside the image"):
        _lib.read_status("ps_zbuffer_scatter_sorted_f32", DEV)
    _lib.read_status("ps_zbuffer_scatter_sorted_f32", DEV)              # cleared by the read
    assert np.array_equal(bits(out.cpu().numpy()), bits(want))


def test_status_word_reports_dropped_points_and_bad_orders():
    """Data errors only the device can see -- a pixel outside the image in the z-buffer scatter, a generation order that is no
    permutation -- raise a bit in the CALLER's status word; ps_read_status turns it into an error (message through
    ps_last_error) and clears it.  The library holds no flag of its own."""
    B, N, H, W = 1, 64, 8, 8
    ys = np.zeros((B, N), np.int32)
    xs = np.zeros((B, N), np.int32)
    ys[0, 5] = H                                           # outside
    v = np.zeros((B, N), np.float32)
    out = torch.full((B, 2, H, W), -2.0, device=DEV)
    winner = torch.empty(B, H, W, dtype=torch.int32, device=DEV)
    dev = [tt(a) for a in (ys, xs, v, v)]
    st = _lib.status_word(DEV)
    _lib.check(_lib.lib().ps_zbuffer_scatter_f32(*[_lib.ptr(a) for a in dev], B, N, H, W, _lib.ptr(out), _lib.ptr(winner), _lib.ptr(st),
                                                 _lib.current_stream()), "ps_zbuffer_scatter_f32")
    with pytest.raises(RuntimeError, match="outside the image"):
        _lib.read_status("scatter", DEV)
    _lib.read_status("scatter", DEV)                       # cleared by the read
    order = torch.arange(16, dtype=torch.int32, device=DEV).view(1, 16).clone()
    order[0, 3] = 99                                       # no permutation of the 4x4 grid
    masks = [torch.empty(1, 9, 16, device=DEV) for _ in range(3)]
    _lib.check(_lib.lib().ps_order_masks_f32(_lib.ptr(order), 1, 4, 4, *[_lib.ptr(m) for m in masks], _lib.ptr(st),
                                             _lib.current_stream()), "ps_order_masks_f32")
    with pytest.raises(RuntimeError, match="no permutation"):
        _lib.read_status("order_masks", DEV)
    _lib.read_status("order_masks", DEV)


def test_depth_manipulator_refuses_sizes_the_reference_literals_do_not_cover():
    from pixelsynth_amd.projection.depth_manipulator import DepthManipulator
    dm = DepthManipulator(128)
    eye = torch.eye(4, device=DEV)[None]
    with pytest.raises(ValueError, match="256x256"):
        dm.project_zbuffer(torch.ones(1, 1, 128, 128, device=DEV), eye, eye, eye, eye)


@functools.lru_cache(maxsize=None)
def manipulated():
    """[(name, inputs, sampler, depth)] of DepthManipulator.project_zbuffer on the fixture's four cases, run once for the tests below"""
    import make_golden_inputs as mgi
    from pixelsynth_amd.projection.depth_manipulator import DepthManipulator
    fx = np.load(os.path.join(GOLD, "zbuffer.npz"))
    out = []
    for name, W, d, cams, RT2 in mgi.zbuffer_cases({str(n): int(fx[f"{n}_seed"]) for n in fx["names"]}):
        dm = DepthManipulator(W)
        smp, dep = dm.project_zbuffer(tt(d), tt(cams["K"]), tt(cams["Kinv"]), tt(cams["Pinv"]), tt(RT2))
        out.append((name, (W, d, cams, RT2), smp.cpu().numpy(), dep.cpu().numpy()))
    assert len(out) == 4
    return out


def test_depth_manipulator_is_the_sequential_mirror_exactly():
    """DepthManipulator.project_zbuffer end to end -- projection kernel, torch's stable sort on the device, scatter kernel --
    against the mirror's projection, a stable argsort of -z and the in-order scatter on the same inputs: both returned tensors
    equal over the whole 256 x 256 arrays, bit for bit.  (tests/test_zbuffer_cpu.py holds that mirror to the reference's own
    outputs, and torch's tie-breaking to numpy's.)"""
    for name, (W, d, cams, RT2), smp, dep in manipulated():
        grid = zo.grid(W)[0].reshape(4, W * W)
        want, wdep, _ = zr.project_zbuffer(d, cams["K"], cams["Kinv"], cams["Pinv"], RT2, grid)
        assert np.array_equal(bits(dep), bits(wdep)), f"{name}: {(bits(dep) != bits(wdep)).sum()} projected depths differ from the mirror's"
        assert np.array_equal(bits(smp), bits(want)), f"{name}: {(bits(smp) != bits(want)).sum()} sampler entries differ from the mirror's"


def test_depth_manipulator_matches_the_reference_outputs():
    fx = np.load(os.path.join(GOLD, "zbuffer.npz"))
    for name, (W, d, cams, RT2), smp, dep in manipulated():
        np.testing.assert_allclose(dep[:, :, ::5, ::5], fx[f"{name}_depth_sub"], rtol=2e-5, atol=2e-5)
        assert np.array_equal(bits(dep[:, :, ::5, ::5]), bits(fx[f"{name}_depth_sub"])), f"{name}: projected depth is not the reference's bits"
        # which point stays on a pixel is an integer decision taken on float products: a z that is a last bit off turns a near-tie
        # of the sort round.  The kernel's products are the fused chains of the reference's bmm on the CPU (mat4_vec_fma of
        # csrc/zbuffer.hip), so the decisions are the reference's: the sampled entries and the filled counts equal, and the row
        # sums, which see every entry, as close as the CPU oracle's
        got, ref = smp[:, :, ::3, ::3], fx[f"{name}_sampler_sub"]
        assert np.array_equal(got, ref), f"{name}: {(got != ref).sum()} of {ref.size} sampler entries differ from the reference"
        np.testing.assert_allclose(smp.astype(np.float64).sum(3), fx[f"{name}_sampler_rowsum"], rtol=0, atol=1e-9)
        filled = np.array([(smp[b, 0] != -2).sum() for b in range(smp.shape[0])])
        assert np.array_equal(filled, fx[f"{name}_filled"])
        # the oracle multiplies with BLAS, whose sums are its own: a few entries in a thousand are granted to that
        want, _ = zo.project_zbuffer(d, cams["K"], cams["Kinv"], cams["Pinv"], RT2)
        assert (smp != want).mean() < 5e-3
