"""Shared by tests/test_splat_bwd_cpu.py and tests/test_splat_bwd_gpu.py: the yardstick of the splat's backward pass.  No test in here,
and nothing of the library is imported.

splat_formula() is the compositing as a torch expression of the CALLER's points and the features, parameterised by dtype, on the hit
lists of the C oracle (oracle.c_oracle.splat_forward through tests/_splat_ref.py): which points a pixel lists, in which order, is
piecewise constant and taken from idx; the squared distances are recomputed from the points so that autograd reaches them.  The clamps
are torch.where selects with the strict convention of include/pixelsynth_splat_bwd.h: the derivative of alpha with respect to the
distance is that of the unclamped expression where 1e-3f < d2 / denom < 1 strictly and exactly 0 elsewhere.  The z of a point is not
used, so its gradient is exactly 0.

project_formula() restates the reference's project_pts (models/projection/z_buffer_manipulator.py:50-83) in torch at any dtype.

The bar of the GPU tests (bar(), kink_points()) is stated here as well, with its reasons:
    g64 = fp64 autograd of the formula, g32 = the same formula in fp32, both on the CPU;  E32 = max |g32 - g64|
    max |g_hip - g64| <= MARGIN * max(E32, FLOOR * max |g64|)
The kernels sum in another order and take their roots and quotients differently from torch's CPU fp32; each evaluation is a sample of the
same unit roundoff, hence the margin of 4; a wrong or missing term is at least 1e-2 of max |g64|, orders above the bar.  E32 / max |g64|
measured on the reference alone: 1e-7 .. 4e-6 for tau >= 1, about 1e-4 for grad_pts at tau = 0.5 (the derivative is unbounded at the
rim of a disc), which is why the accuracy of grad_pts is not pinned at tau < 1.

ROUTE_CASES are the cases with more feature channels than the operator test's (OPERATOR_CASE_IDS: 3, 5 or 8): 13 to 130, the model's own
64 among them, where k_splat_bwd_pixels carries q_k over several chunks of 8 channels (pixel_chunks) and k_splat_bwd_points walks a point's
box once per 64 channels (box_walks).  The kernel adds q_k = <g, f> over the C channels as one ascending chain, torch's fp32 sum does
not; E32 / max |g64| of the reference alone stays at 1.5e-7 .. 2.3e-6 for them and the same bar holds with MARGIN 4 as it is (largest
max |g_hip - g64| / E32 on the MI355X: 1.78, grad_pts at C = 130), so E32 is the one fp32 evaluation's as for every other case.
"""
import numpy as np
import torch

import _splat_ref as sr

MARGIN = 4.0
FLOOR = 1e-6
KINK = 1e-4            # a hit this close to a clamp bound (relative at 1e-3, absolute at 1) can fall on either side in fp32 and fp64
EPS = 1e-2             # z_buffer_manipulator.py:8
D_LO = float(np.float32(1e-3))
T_MIN = float(np.float32(1e-4))


# The cases of the operator test (tests/test_splat_bwd_gpu.py: test_gradients_against_fp64_autograd), by id in _splat_ref.CASES: 3, 5 or 8
# feature channels, every one
OPERATOR_CASE_IDS = ("division_S40", "division_S40_scale50", "wsum_tau1", "wsum_tau2", "wsumnorm_tau1", "wsumnorm_tau2", "tau2_S40",
                     "channels_5", "channels_8", "partial_tiles_S20", "rad_pow1_C3", "rad_pow3_C5", "footprint_gt9", "sort_len_129",
                     "tau0.5_S40")
QCH = 8                # csrc/splat_bwd.hip's QCH: channels of grad_out k_splat_bwd_pixels keeps while it walks a list once
LANES = 64             # channels k_splat_bwd_points owns in one walk of a point's box


def pixel_chunks(C):
    """Trips of k_splat_bwd_pixels' channel loop: q_k is carried from chunk to chunk through the plane"""
    return -(-C // QCH)


def box_walks(C):
    """Walks of a point's box in k_splat_bwd_points when grad_feat is asked for: one per 64 channels, the points' gradient in the first"""
    return -(-C // LANES)


def _route(id, C, seed, acc="alphacomposite", tau=1.0, S=24, N=800, K=8, r=3):
    return sr._small_case(id, S, N, K, r, ksize=3, C=C, acc=acc, tau=tau, seed=seed)


# More channels than a chunk and than a wave (tests/test_train_routes2_cpu.py asserts what each reaches, tests/test_train_routes2_gpu.py
# runs them).  A tuple of its own: the forward tests iterate over _splat_ref.CASES.  N = 300: most lists end in -1 before K.
ROUTE_CASES = (
    _route("bwd_C13_wsumnorm", 13, 401, acc="wsumnorm"),      # two chunks, the last of 5; wq sums a q made of both
    _route("bwd_C16", 16, 402, N=300),                        # two full chunks
    _route("bwd_C64", 64, 403),                               # eight chunks; every lane of the point kernel owns a channel
    _route("bwd_C70_tau2", 70, 404, tau=2.0),                 # nine chunks, the last of 6; a second walk with 6 lanes live
    _route("bwd_C130_wsum", 130, 405, acc="wsum", S=16, N=300, K=4, r=2.5),      # three walks, the last with 2 lanes live
    _route("bwd_K1", 9, 406, K=1),                            # both walks of a list one step long
)


def splat_formula(pts, feat, idx, S, radius_px, rad_pow, tau, acc):
    """pts (B,N,3) and feat (B,C,N) torch tensors of one dtype (the caller's points, before the negation), idx (B,S,S,K) the oracle's
    packed indices (b*N + n, -1 behind the last hit) as a numpy array or tensor -> features (B,C,S,S) of that dtype"""
    B, N, _ = pts.shape
    dt = pts.dtype
    idx = torch.as_tensor(np.array(idx)).long()
    hit = idx >= 0
    n = torch.where(hit, idx % N, torch.zeros_like(idx))                       # (B,S,S,K)
    centre = -1.0 + (2.0 * (S - 1 - torch.arange(S, dtype=dt)) + 1.0) / S       # pixel i is tested against PixToNdc(S - 1 - i)
    flat = n.reshape(B, -1)
    px = torch.gather(-pts[..., 0], 1, flat).reshape(n.shape)
    py = torch.gather(-pts[..., 1], 1, flat).reshape(n.shape)
    dx, dy = px - centre.view(1, 1, S, 1), py - centre.view(1, S, 1, 1)
    d2 = dx * dx + dy * dy
    r = d2 / torch.tensor(float(sr.denom64(S, radius_px, rad_pow)), dtype=dt)
    inside = (r > D_LO) & (r < 1.0)
    d = torch.where(inside, r, r.detach().clamp(D_LO, 1.0))                    # a select: no gradient where the clamp holds
    a = (1.0 - torch.sqrt(d)) ** float(tau)
    a = torch.where(hit, a, torch.zeros_like(a))
    if acc == "alphacomposite":
        w = a * torch.cat([torch.ones_like(a[..., :1]), torch.cumprod(1.0 - a, dim=-1)[..., :-1]], dim=-1)
    elif acc == "wsum":
        w = a
    elif acc == "wsumnorm":
        t = a.sum(-1, keepdim=True)
        w = a / torch.where(t >= T_MIN, t, torch.full_like(t, T_MIN).detach())
    else:
        raise KeyError(acc)
    f = torch.gather(feat, 2, flat.unsqueeze(1).expand(B, feat.size(1), -1)).reshape(B, feat.size(1), *n.shape[1:])   # (B,C,S,S,K)
    return (w.unsqueeze(1) * f).sum(-1)


def case_gradients(c, pts, feat, idx, grad_out, dtype):
    """(features, grad_pts, grad_feat) of the formula at `dtype` on the CPU for a case of _splat_ref.CASES; float64 numpy arrays out"""
    p = torch.tensor(np.asarray(pts)).to(dtype).requires_grad_()
    f = torch.tensor(np.asarray(feat)).to(dtype).requires_grad_()
    out = splat_formula(p, f, idx, c.S, c.r, c.rad_pow, c.tau, c.acc)
    gp, gf = torch.autograd.grad(out, (p, f), torch.tensor(np.asarray(grad_out)).to(dtype))
    return out.detach().double().numpy(), gp.double().numpy(), gf.double().numpy()


def project_formula(depth, K, Kinv, RT1inv, RT2, W):
    """Reference :50-83 at the dtype of depth: depth (B,1,W*W) -> sampler (B,3,W*W)"""
    dt = depth.dtype
    axis = torch.arange(W, dtype=dt) / float(W - 1) * 2 - 1
    xs, ys = axis.view(1, W).expand(W, W).reshape(-1), axis.view(W, 1).expand(W, W).reshape(-1)
    one = torch.ones(W * W, dtype=dt)
    xyzs = torch.stack((xs, -ys, -one, one)).unsqueeze(0)
    coors = xyzs * depth
    coors = torch.cat([coors[:, :3], torch.ones_like(coors[:, 3:])], 1)          # projected_coors[:, -1, :] = 1
    xy = K.bmm(RT2.bmm(RT1inv).bmm(Kinv.bmm(coors)))
    mask = (xy[:, 2:3].abs() < EPS).detach()
    zs = torch.where(mask, torch.full_like(xy[:, 2:3], EPS), xy[:, 2:3])          # zs[mask] = EPS
    sampler = torch.cat((xy[:, 0:2] / -zs, zs), 1)
    sampler = torch.where(mask.expand(-1, 3, -1), torch.full_like(sampler, -10.0), sampler)
    return sampler * torch.tensor([1.0, -1.0, -1.0], dtype=dt).view(1, 3, 1)


def bar(g64, g32):
    """-> (the bound on max |g - g64|, E32)"""
    e32 = float(np.abs(g32 - g64).max())
    return MARGIN * max(e32, FLOOR * float(np.abs(g64).max())), e32


def hit_points(idx, B, N):
    """(B,N) bool: the points that are in any pixel's list"""
    seen = np.zeros(B * N, bool)
    seen[idx[idx >= 0]] = True
    return seen.reshape(B, N)


def kink_points(c, idx, dist, B, N):
    """(B,N) bool: the points with a hit within KINK of a clamp bound (relative at the lower, absolute at the upper), by the oracle's dist"""
    r = dist.astype(np.float64) / sr.denom64(c.S, c.r, c.rad_pow)
    near = (idx >= 0) & ((np.abs(r - D_LO) <= KINK * D_LO) | (np.abs(r - 1.0) <= KINK))
    out = np.zeros(B * N, bool)
    out[idx[near]] = True
    return out.reshape(B, N)
