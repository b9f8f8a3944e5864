"""The homography consistency score of two generated views (the reference's calc_errors_consistency_homography.py) on the ROCm device:
the binding of csrc/consistency.hip, and the homography fit on the host.

consistency_rows(img1, img2, mask1, mask2, H12=None, H21=None, points=None, pnet=None) -> (B, 3) f32 tensor, columns COLUMNS[:3]
(psnr_vis_0, psnr_vis_1, psnr_vis), or (B, 6) with a PNet `pnet` (COLUMNS: percsim_vis_0, percsim_vis_1, percsim_vis added).
Direction 0 warps view 2 into view 1's frame (H21) and compares it with view 1 under mask 1; direction 1 warps view 1 into view 2's
frame (H12) under mask 2 (:87-98).  Each direction's PSNR is clamped at 100; psnr_vis and percsim_vis are 0.5 (dir0 + dir1) (:103-105).
img1, img2 (B, 3, H, W) uint8 or float32 in [0, 1], any strides; mask1, mask2 (B, 1, H, W) uint8 (g / 255, the grayscale PNG) or
float32.  H12 / H21: (B, 3, 3) homographies in pixel units, view 1 -> view 2 and view 2 -> view 1 (cv2's convention: dst ~ H src);
or points = (reproj1, reproj2), the reference's raw point arrays (B arrays of (n, >= 2), or (B, n, >= 2)), fitted here as the
reference fits them (fit_points).  Everything is checked before the first launch; a CPU tensor is an error (no CPU fallback).

find_homography(src, dst) restates cv2.findHomography with method 0 (HomographyEstimatorCallback::runKernel, then 10
Levenberg-Marquardt iterations, modules/calib3d/src/fundam.cpp and levmarq.cpp of OpenCV 4.x) in batched fp64 numpy.  The warp is
warpPerspective with INTER_LINEAR and BORDER_CONSTANT 0 (csrc/consistency.hip).
"""
import numpy as np
import torch

from . import _images, _lib
from .networks import f16x3
from .perceptual import check_pnet, network_pass, pairs_per_pass

COLUMNS = ("psnr_vis_0", "psnr_vis_1", "psnr_vis", "percsim_vis_0", "percsim_vis_1", "percsim_vis")
MAPPING = ("R", "L", "U", "D", "UL", "UR", "DR", "DL")    # :20-22, the direction names of the view files
NO_PERCSIM, PERCSIM, PERCSIM_RAW = 0, 1, 2                # PS_CONSISTENCY_*
_LM_ITERS = 10


def _labels(items, B):
    return list(range(B)) if items is None else list(items)


def _dlt(src, dst, labels):
    """HomographyEstimatorCallback::runKernel, batched: src, dst (B, n, 2) fp64 -> (B, 3, 3) with H[2, 2] = 1."""
    B, n = src.shape[:2]
    cM, cm = src.mean(1), dst.mean(1)                                       # (B, 2)
    sM, sm = np.abs(src - cM[:, None]).sum(1), np.abs(dst - cm[:, None]).sum(1)
    eps = np.finfo(np.float64).eps
    for i in range(B):
        if (sM[i] < eps).any() or (sm[i] < eps).any():
            raise ValueError(f"find_homography: item {labels[i]}: the points of one set coincide along an axis (degenerate set)")
    sM, sm = n / sM, n / sm                                                 # per axis: n / sum |x - c|  (L1, not the RMS)
    X, Y = ((src - cM[:, None]) * sM[:, None]).transpose(2, 0, 1)           # (B, n) each
    x, y = ((dst - cm[:, None]) * sm[:, None]).transpose(2, 0, 1)
    one, zero = np.ones_like(X), np.zeros_like(X)
    Lx = np.stack([X, Y, one, zero, zero, zero, -x * X, -x * Y, -x], 2)    # (B, n, 9)
    Ly = np.stack([zero, zero, zero, X, Y, one, -y * X, -y * Y, -y], 2)
    LtL = np.einsum("bnj,bnk->bjk", Lx, Lx) + np.einsum("bnj,bnk->bjk", Ly, Ly)
    _, V = np.linalg.eigh(LtL)
    H0 = V[:, :, 0].reshape(B, 3, 3)                                         # the eigenvector of the smallest eigenvalue
    inv_norm = np.zeros((B, 3, 3))
    inv_norm[:, 0, 0], inv_norm[:, 0, 2] = 1.0 / sm[:, 0], cm[:, 0]
    inv_norm[:, 1, 1], inv_norm[:, 1, 2] = 1.0 / sm[:, 1], cm[:, 1]
    inv_norm[:, 2, 2] = 1.0
    norm2 = np.zeros((B, 3, 3))
    norm2[:, 0, 0], norm2[:, 0, 2] = sM[:, 0], -cM[:, 0] * sM[:, 0]
    norm2[:, 1, 1], norm2[:, 1, 2] = sM[:, 1], -cM[:, 1] * sM[:, 1]
    norm2[:, 2, 2] = 1.0
    H = inv_norm @ H0 @ norm2
    return H / H[:, 2:3, 2:3]


def _residuals(h, src, dst, jac=False):
    """HomographyRefineCallback::compute: h (B, 8) -> err (B, 2n) (x, y interleaved) and, with jac, J (B, 2n, 8)."""
    Mx, My = src[..., 0], src[..., 1]
    ww = h[:, 6:7] * Mx + h[:, 7:8] * My + 1.0
    ww = np.where(np.abs(ww) > np.finfo(np.float64).eps, 1.0 / np.where(ww == 0, 1.0, ww), 0.0)
    xi = (h[:, 0:1] * Mx + h[:, 1:2] * My + h[:, 2:3]) * ww
    yi = (h[:, 3:4] * Mx + h[:, 4:5] * My + h[:, 5:6]) * ww
    err = np.stack([xi - dst[..., 0], yi - dst[..., 1]], 2).reshape(len(h), -1)
    if not jac:
        return err
    B, n = Mx.shape
    J = np.zeros((B, n, 2, 8))
    J[:, :, 0, 0], J[:, :, 0, 1], J[:, :, 0, 2] = Mx * ww, My * ww, ww
    J[:, :, 0, 6], J[:, :, 0, 7] = -Mx * ww * xi, -My * ww * xi
    J[:, :, 1, 3], J[:, :, 1, 4], J[:, :, 1, 5] = Mx * ww, My * ww, ww
    J[:, :, 1, 6], J[:, :, 1, 7] = -Mx * ww * yi, -My * ww * yi
    return err, J.reshape(B, 2 * n, 8)


def _pinv_eig(A):
    """cv::invert(A, DECOMP_EIG) of symmetric A (B, n, n), also what solve(A, b, DECOMP_EIG) applies to b: the pseudo-inverse of the
    eigen-decomposition, eigenvalues at or below 2 DBL_EPSILON sum(w) taken as zero (SVBkSb's threshold)."""
    w, V = np.linalg.eigh(A)
    thr = 2.0 * np.finfo(np.float64).eps * np.abs(w).sum(1, keepdims=True)
    keep = w > thr
    inv = np.where(keep, 1.0 / np.where(keep, w, 1.0), 0.0)
    return np.einsum("bij,bj,bkj->bik", V, inv, V)


def _refine(H, src, dst, iters=_LM_ITERS):
    """createLMSolver(HomographyRefineCallback(src, dst), 10)->run(H8): the LM solver of OpenCV's levmarq.cpp on the 8 free entries,
    each item on its own schedule (a step is kept only when it lowers the summed squared error)."""
    eps = np.finfo(np.float32).eps                    # the solver's default epsilon (FLT_EPSILON)
    dbl = np.finfo(np.float64).eps
    B = len(H)
    x = H.reshape(B, 9)[:, :8].copy()
    r, J = _residuals(x, src, dst, True)
    S = (r * r).sum(1)
    A = np.einsum("bij,bik->bjk", J, J)
    v = np.einsum("bij,bi->bj", J, r)
    D = np.diagonal(A, axis1=1, axis2=2).copy()
    lam, lc = np.ones(B), np.full(B, 0.75)
    live = np.ones(B, bool)
    it = 0
    while live.any():
        Ap = A + lam[:, None, None] * (D[:, :, None] * np.eye(8))
        d = np.zeros_like(x)                          # solve(Ap, v, d, DECOMP_EIG); finished items take no step
        d[live] = np.einsum("bij,bj->bi", _pinv_eig(Ap[live]), v[live])
        xd = x - d
        rd = _residuals(xd, src, dst)
        Sd = np.where(live, (rd * rd).sum(1), S)
        temp = -np.einsum("bjk,bk->bj", A, d) + 2.0 * v
        dS = (d * temp).sum(1)
        R = (S - Sd) / np.where(np.abs(dS) > dbl, dS, 1.0)
        hi, lo = live & (R > 0.75), live & (R < 0.25)
        lam = np.where(hi, lam * 0.5, lam)
        lam = np.where(hi & (lam < lc), 0.0, lam)
        if lo.any():
            t = (d * v).sum(1)
            nu = np.clip((Sd - S) / np.where(np.abs(t) > dbl, t, 1.0) + 2.0, 2.0, 10.0)
            for i in np.nonzero(lo & (lam == 0))[0]:
                Ai = _pinv_eig(A[i][None])[0]
                lam[i] = lc[i] = 1.0 / max(dbl, float(np.abs(np.diag(Ai)).max()))
                nu[i] *= 0.5
            lam = np.where(lo, lam * nu, lam)
        take = live & (Sd < S)
        if take.any():
            x[take], S[take] = xd[take], Sd[take]
            r2, J2 = _residuals(x[take], src[take], dst[take], True)
            r[take] = r2
            A[take] = np.einsum("bij,bik->bjk", J2, J2)
            v[take] = np.einsum("bij,bi->bj", J2, r2)
        it += 1
        live &= (it < iters) & (np.abs(d).max(1) >= eps) & (np.abs(r).max(1) >= eps)
    out = np.concatenate([x, np.ones((B, 1))], 1).reshape(B, 3, 3)
    return out


def find_homography(src, dst, items=None):
    """cv2.findHomography(src, dst) with method 0, batched in fp64: src, dst (n, 2) or (B, n, 2) -> (3, 3) or (B, 3, 3), dst ~ H src,
    H[2, 2] = 1.  The DLT on points normalised per axis (centred on the mean, scaled by n / sum |x - c|), then, for n > 4, 10
    Levenberg-Marquardt iterations on the forward reprojection error sum |dst - H(src)|^2.  Fewer than 4 points, or a degenerate set
    (coincident or collinear points), raise ValueError naming the item (`items`: the labels to name, default the batch index); cv2
    returns an empty matrix there.  (cv2 rounds the points to fp32 first: fit_points does so, this function does not.)"""
    src, dst = np.asarray(src, np.float64), np.asarray(dst, np.float64)
    single = src.ndim == 2
    if single:
        src, dst = src[None], dst[None]
    if src.ndim != 3 or src.shape[2] != 2 or src.shape != dst.shape:
        raise ValueError(f"find_homography: src and dst must be (n, 2) or (B, n, 2) of one shape, got {src.shape} and {dst.shape}")
    B, n = src.shape[:2]
    labels = _labels(items, B)
    if n < 4:
        raise ValueError(f"find_homography: item {labels[0] if B else '?'}: {n} point(s), at least 4 required")
    for i in range(B):
        for pts in (src[i], dst[i]):
            c = pts - pts.mean(0)
            sv = np.linalg.svd(c, compute_uv=False)
            if not np.isfinite(sv).all() or sv[1] <= 1e-9 * max(sv[0], 1e-300):
                raise ValueError(f"find_homography: item {labels[i]}: the points are collinear (degenerate set)")
    H = _dlt(src, dst, labels)
    if n > 4:
        H = _refine(H, src, dst)
    return H[0] if single else H


def points_to_pixels(npy):
    """Steps of :82-86 on one raw reference-point array (n, >= 2): (p * 0.5 + 0.5) * 255 in the array's own dtype, the literal 255
    for both axes, x flipped as 255 - x; columns 0 and 1.  Then the fp32 rounding cv2.findHomography applies to its input."""
    p = (np.asarray(npy) * .5 + .5) * 255
    p[:, 0] = 255 - p[:, 0]
    return p[:, :2].astype(np.float32)


def fit_points(reproj1, reproj2, items=None):
    """:82-88 for a batch of items: the reference's raw point arrays -> (H12, H21) (B, 3, 3) fp64, H12 = findHomography(src, dst) and
    H21 = findHomography(dst, src), fitted separately (H21 is not inv(H12); the two differ when the points are noisy)."""
    if len(reproj1) != len(reproj2):
        raise ValueError(f"fit_points: {len(reproj1)} and {len(reproj2)} point arrays")
    labels = _labels(items, len(reproj1))
    src = [points_to_pixels(p) for p in reproj1]
    dst = [points_to_pixels(p) for p in reproj2]
    H12, H21 = np.empty((len(src), 3, 3)), np.empty((len(src), 3, 3))
    for i, (s, d) in enumerate(zip(src, dst)):       # (items may differ in point count)
        if s.shape != d.shape:
            raise ValueError(f"fit_points: item {labels[i]}: {s.shape[0]} and {d.shape[0]} points")
        H12[i] = find_homography(s, d, [labels[i]])
        H21[i] = find_homography(d, s, [labels[i]])
    return H12, H21


def invert_map(H):
    """cv::invert of a 3 x 3 fp64 matrix with DECOMP_LU (the adjugate over det3), as warpPerspective inverts its map: (B, 3, 3)."""
    S = np.asarray(H, np.float64)
    a = lambda i, j: S[:, i, j]
    det = a(0, 0) * (a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1)) - a(0, 1) * (a(1, 0) * a(2, 2) - a(1, 2) * a(2, 0)) \
        + a(0, 2) * (a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0))
    if (det == 0).any():
        raise ValueError(f"a homography is singular (items {np.nonzero(det == 0)[0].tolist()})")
    d = 1.0 / det
    t = np.stack([(a(1, 1) * a(2, 2) - a(1, 2) * a(2, 1)) * d, (a(0, 2) * a(2, 1) - a(0, 1) * a(2, 2)) * d,
                  (a(0, 1) * a(1, 2) - a(0, 2) * a(1, 1)) * d, (a(1, 2) * a(2, 0) - a(1, 0) * a(2, 2)) * d,
                  (a(0, 0) * a(2, 2) - a(0, 2) * a(2, 0)) * d, (a(0, 2) * a(1, 0) - a(0, 0) * a(1, 2)) * d,
                  (a(1, 0) * a(2, 1) - a(1, 1) * a(2, 0)) * d, (a(0, 1) * a(2, 0) - a(0, 0) * a(2, 1)) * d,
                  (a(0, 0) * a(1, 1) - a(0, 1) * a(1, 0)) * d], 1)
    return t.reshape(-1, 3, 3)


def _check(img1, img2, mask1, mask2, pnet):
    """-> (B, H, W, the device)"""
    B, _, H, W = _images.check_images({"img1": img1, "img2": img2}, (3,), "(B, 3, H, W)")
    for name, m in (("mask1", mask1), ("mask2", mask2)):
        _images.check_mask(name, m, (B, 1, H, W), _images.CODED)
    if mask1.dtype != mask2.dtype:
        raise TypeError(f"mask1 and mask2 must have one dtype, got {mask1.dtype} and {mask2.dtype}")
    if pnet is not None:
        check_pnet(pnet)
    return B, H, W, _images.same_device(img1=img1, img2=img2, mask1=mask1, mask2=mask2)


def _maps(B, H12, H21, points):
    """-> (B, 2, 9) fp64: the inverted maps of direction 0 (H21) and direction 1 (H12)"""
    if points is not None:
        if H12 is not None or H21 is not None:
            raise ValueError("pass either H12 and H21 or points, not both")
        H12, H21 = fit_points(*points)
    elif H12 is None or H21 is None:
        raise ValueError("H12 and H21 (or points) are required")
    H12, H21 = (np.asarray(h.cpu().numpy() if torch.is_tensor(h) else h, np.float64) for h in (H12, H21))
    for name, h in (("H12", H12), ("H21", H21)):
        if h.shape != (B, 3, 3):
            raise ValueError(f"{name} must be (B, 3, 3) = {(B, 3, 3)}, got {h.shape}")
    return np.ascontiguousarray(np.stack([invert_map(H21), invert_map(H12)], 1).reshape(B, 2, 9))


def _launch(img1, img2, mask1, mask2, maps, mode, pin, psnr):
    B, _, H, W = img1.shape
    ws, nbytes = _images.workspace("ps_consistency_workspace_bytes", B, H, W, device=img1.device)
    _lib.call("ps_consistency", img1, _images.strides(img1), img2, _images.strides(img2), _images.DTYPES[img1.dtype], mask1, mask2,
              _images.DTYPES[mask1.dtype], maps, B, H, W, mode, pin, psnr, ws, nbytes)


def consistency_rows(img1, img2, mask1, mask2, H12=None, H21=None, points=None, pnet=None):
    B, H, W, dev = _check(img1, img2, mask1, mask2, pnet)
    mask1, mask2 = mask1.contiguous(), mask2.contiguous()
    maps = torch.from_numpy(_maps(B, H12, H21, points)).to(dev)
    probe = torch.empty((1, 3, H, W), dtype=torch.float32, device=dev)   # what PercSim's HIP path takes (no data is read)

    def run():
        out = torch.empty(B, 6 if pnet is not None else 3, dtype=torch.float32, device=dev)
        hip = pnet is not None and pnet.hip_takes(probe, probe)
        # items per launch; with a PNet, per network pass (2 pairs each)
        per = _images.MAX_B if pnet is None else max(1, min(_images.MAX_B, pairs_per_pass(H, W) // 2))
        with torch.cuda.device(dev):
            layers = pnet.hip_layers(dev) if hip else None
            for b0, b1 in _images.batches(B, per):
                n = b1 - b0
                psnr = torch.empty(n, 2, dtype=torch.float32, device=dev)
                pin = None if pnet is None else torch.empty((4 * n, H, W, 4), dtype=torch.float32, device=dev)
                mode = NO_PERCSIM if pnet is None else (PERCSIM if hip else PERCSIM_RAW)
                _launch(img1[b0:b1], img2[b0:b1], mask1[b0:b1], mask2[b0:b1], maps[b0:b1], mode, pin, psnr)
                out[b0:b1, 0:2] = psnr
                if pnet is not None:
                    if hip:
                        _, total = network_pass(layers, pin.permute(0, 3, 1, 2), 2 * n, H, W)
                    else:                                                  # PNet.forward's torch formula on the same inputs
                        x = pin[..., :3].permute(0, 3, 1, 2)
                        total = pnet.torch_forward(x[:2 * n], x[2 * n:])
                    out[b0:b1, 3:5] = total.view(n, 2)
        # 0.5 (dir0 + dir1): exact in fp64 for fp32 operands, then rounded once
        out[:, 2] = (0.5 * (out[:, 0].double() + out[:, 1].double())).float()
        if pnet is not None:
            out[:, 5] = (0.5 * (out[:, 3].double() + out[:, 4].double())).float()
        return out
    with torch.no_grad():
        return f16x3.checked(dev, run)
