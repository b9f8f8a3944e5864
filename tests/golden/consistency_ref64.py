"""The homography consistency cases of tests/golden/consistency.npz and an fp64 numpy restatement of the reference's
calc_errors_consistency_homography.py, steps 1-9: points to pixels, the two fits (pixelsynth_amd.consistency.find_homography, tested
on its own), warpPerspective (INTER_LINEAR, BORDER_CONSTANT 0; the fixed-point source position exactly, the bilinear sum in fp64),
the masked comparison and PSNR_vis clamped at 100 per direction, and PercSim_vis's inputs (BGR-ordered, in [0, 1]).  The inputs the
reference forms in fp32 (u = x / 255, try = u * 255, m = g / 255) are formed in fp32 here too; everything after them in fp64.
Shared by make_consistency_golden.py and the consistency tests."""
import numpy as np

from pixelsynth_amd import consistency as C, synthetic as syn

S = 256
# name, seed, B, rotation (degrees: yaw, pitch, roll), point noise (pixels), mask kind: "valid" (the pixels whose preimage is inside
# the other view, as a 0/255 grayscale PNG holds it), "fractional" (U(0, 1) fp32), "empty" (all zero)
CASES = [
    ("exact_small", 21, 2, (3.0, -2.0, 1.0), 0.0, "valid"),
    ("noisy", 22, 2, (-4.0, 3.0, -2.0), 0.7, "valid"),
    ("fractional", 23, 1, (2.0, 2.0, 0.0), 0.3, "fractional"),
    ("empty_mask", 24, 1, (1.0, 0.0, 0.0), 0.0, "empty"),
]
N_POINTS = 24


def K():
    return np.array([[256.0, 0.0, 127.5], [0.0, 256.0, 127.5], [0.0, 0.0, 1.0]])


def rotation_homography(deg):
    """K R K^-1 of a rotation by yaw, pitch, roll (degrees): a pure-rotation homography in pixel units."""
    R = syn.euler_to_R(np.radians(np.asarray(deg, np.float64)))
    R = np.asarray(R, np.float64).reshape(3, 3)
    return K() @ R @ np.linalg.inv(K())


def smooth_view(seed, B):
    """(B, 3, S, S) uint8: box-blurred noise, smooth enough for a warp to keep most of its content"""
    a, _ = syn.metric_pair(seed, B, 3, S, S, "noise_blur")
    for _ in range(3):
        p = np.pad(a, ((0, 0), (0, 0), (2, 2), (2, 2)), mode="edge")
        a = sum(p[:, :, dy:dy + S, dx:dx + S] for dy in range(5) for dx in range(5)) / np.float32(25.0)
    lo, hi = a.min(), a.max()
    return np.clip(np.round((a - lo) / (hi - lo) * 255.0), 0, 255).astype(np.uint8)


def to_raw(px):
    """Pixel positions (n, 2) -> the reference's raw point array (n, 3) that points_to_pixels maps back (x flipped, the 255 literal)"""
    raw = np.zeros((len(px), 3))
    raw[:, 0] = ((255.0 - px[:, 0]) / 255.0 - 0.5) / 0.5
    raw[:, 1] = (px[:, 1] / 255.0 - 0.5) / 0.5
    raw[:, 2] = 1.0
    return raw


def apply_h(H, pts):
    q = np.c_[pts, np.ones(len(pts))] @ H.T
    return q[:, :2] / q[:, 2:]


def case_inputs(case):
    """-> dict: view1, view2 (B, 3, S, S) u8; mask1, mask2 (B, 1, S, S) u8 or f32; reproj1, reproj2 (B, n, 3) fp64; Htrue (B, 3, 3)"""
    name, seed, B, deg, noise, mkind = case
    rs = np.random.RandomState(seed)
    Ht = np.stack([rotation_homography(np.asarray(deg) * (1.0 + 0.25 * b)) for b in range(B)])
    view1 = smooth_view(seed, B)
    view2 = np.empty_like(view1)
    for b in range(B):    # view 2: view 1 seen through the rotation (the fp64 warp of its fp32 values, rounded to 8 bits)
        w = warp64(try_bgr(view1[b]), C.invert_map(Ht[b][None])[0].ravel())[:, :, ::-1]
        view2[b] = np.clip(np.round(w), 0, 255).astype(np.uint8).transpose(2, 0, 1)
    r1, r2 = [], []
    for b in range(B):
        src = rs.uniform(20, 235, (N_POINTS, 2))
        dst = apply_h(Ht[b], src) + noise * rs.randn(N_POINTS, 2)
        r1.append(to_raw(src))
        r2.append(to_raw(dst))
    if mkind == "fractional":
        m1, m2 = (rs.rand(B, 1, S, S).astype(np.float32) for _ in range(2))
    elif mkind == "empty":
        m1 = m2 = np.zeros((B, 1, S, S), np.uint8)
    else:
        m1 = np.stack([valid_mask(np.linalg.inv(Ht[b]))[None] for b in range(B)])   # frame-1 pixels seen by view 2
        m2 = np.stack([valid_mask(Ht[b])[None] for b in range(B)])
    return dict(view1=view1, view2=view2, mask1=m1, mask2=m2, reproj1=np.stack(r1), reproj2=np.stack(r2), Htrue=Ht)


def valid_mask(H):
    """0/255 uint8 (S, S): output pixels whose preimage under H lies inside the frame"""
    yy, xx = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64), indexing="ij")
    q = apply_h(np.linalg.inv(H), np.c_[xx.ravel(), yy.ravel()]).reshape(S, S, 2)
    ok = (q[..., 0] >= 0) & (q[..., 0] <= S - 1) & (q[..., 1] >= 0) & (q[..., 1] <= S - 1)
    return np.where(ok, 255, 0).astype(np.uint8)


def unit(x):
    """TF.to_tensor's values: u8 -> fl32(x / 255); fp32 as it is"""
    return (x.astype(np.float32) / np.float32(255.0)).astype(np.float32) if x.dtype == np.uint8 else x.astype(np.float32)


def try_bgr(view):
    """(3, H, W) -> (H, W, 3) fp32 BGR, fl32(u * 255): what the reference feeds to warpPerspective (:76-80)"""
    return (unit(view) * np.float32(255.0)).astype(np.float32).transpose(1, 2, 0)[:, :, ::-1]


def source_positions(Minv, H, W):
    """The fixed-point source position of every output pixel (WarpPerspectiveInvoker) -> (sx, sy, fx, fy) int arrays (H, W)"""
    M = np.asarray(Minv, np.float64)
    bh0 = min(16, H)
    bw0 = min(1024 // bh0, W)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    xb = (xx // bw0) * bw0
    x1 = (xx - xb).astype(np.float64)
    xb, y = xb.astype(np.float64), yy.astype(np.float64)
    X0 = M[0] * xb + M[1] * y + M[2]
    Y0 = M[3] * xb + M[4] * y + M[5]
    W0 = M[6] * xb + M[7] * y + M[8]
    Wd = W0 + M[6] * x1
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        Wd = np.where(Wd != 0, 32.0 / np.where(Wd != 0, Wd, 1.0), 0.0)
        fX, fY = (X0 + M[0] * x1) * Wd, (Y0 + M[3] * x1) * Wd
    hi, lo = float(2 ** 31 - 1), float(-2 ** 31)

    def rnd(v):
        v = np.where(v < hi, v, hi)
        v = np.where(lo < v, v, lo)
        return np.rint(v).astype(np.int64)
    X, Y = rnd(fX), rnd(fY)
    return np.clip(X >> 5, -32768, 32767), np.clip(Y >> 5, -32768, 32767), X & 31, Y & 31


def warp64(img, Minv):
    """warpPerspective(img (H, W, 3) fp32, ...) with the inverted map Minv (9,): INTER_LINEAR, BORDER_CONSTANT 0, the bilinear sum of
    the exact fp32 table weights in fp64 -> (H, W, 3) fp64"""
    H, W = img.shape[:2]
    sx, sy, fx, fy = source_positions(Minv, H, W)
    tx, ty = fx / 32.0, fy / 32.0
    w = ((1 - ty) * (1 - tx), (1 - ty) * tx, ty * (1 - tx), ty * tx)
    out = np.zeros((H, W, 3))
    for k, (dx, dy) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
        X, Y = sx + dx, sy + dy
        ok = (X >= 0) & (X < W) & (Y >= 0) & (Y < H)
        v = np.where(ok[..., None], img[np.clip(Y, 0, H - 1), np.clip(X, 0, W - 1)].astype(np.float64), 0.0)
        out += v * w[k][..., None]
    return out


def mask_unit(m):
    """(1, H, W) u8 or f32 -> (H, W) fp32: fl32(g / 255) or the value"""
    return unit(m[0])


def direction64(src_view, ref_view, mask, Minv):
    """One direction: src warped into the frame of ref -> (psnr clamped, warped (H, W, 3) BGR fp64, a, b (3, H, W) fp64 in [0, 1] BGR:
    PercSim_vis's two inputs before the * 2 - 1)"""
    warped = warp64(try_bgr(src_view), Minv)
    m = mask_unit(mask).astype(np.float64)[..., None]
    a = warped * m / 255.0
    b = m * unit(ref_view).transpose(1, 2, 0)[:, :, ::-1].astype(np.float64)
    num = (((a - b) ** 2) * m).sum()
    den = 3.0 * max(m.sum(), 1.0)
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(1.0 / (num / den))
    return min(psnr, 100.0), warped, a.transpose(2, 0, 1), b.transpose(2, 0, 1)


def item64(view1, view2, mask1, mask2, H12, H21):
    """-> (psnr (2,), [a, b] per direction): direction 0 warps view 2 by H21 into frame 1 under mask 1, direction 1 view 1 by H12"""
    d0 = direction64(view2, view1, mask1, C.invert_map(H21[None])[0].ravel())
    d1 = direction64(view1, view2, mask2, C.invert_map(H12[None])[0].ravel())
    return np.array([d0[0], d1[0]]), [(d0[2], d0[3]), (d1[2], d1[3])]


def case64(case, inputs=None):
    """-> (H12, H21 (B, 3, 3), psnr (B, 2) fp64 clamped per direction) of a case, the fits from its raw points"""
    z = case_inputs(case) if inputs is None else inputs
    H12, H21 = C.fit_points(list(z["reproj1"]), list(z["reproj2"]))
    psnr = np.stack([item64(z["view1"][b], z["view2"][b], z["mask1"][b], z["mask2"][b], H12[b], H21[b])[0]
                     for b in range(len(H12))])
    return H12, H21, psnr
