"""Shared by tests/test_consistency_twin_cpu.py and tests/test_consistency_shapes_gpu.py: a float32 numpy twin of one direction of
k_consistency_tiles (pixelsynth_amd/csrc/consistency.hip), the finish kernel's formula, PNet's standardisation, OpenCV's block walk
written as loops, and the table of shapes, maps, views and masks the two tests walk.  No test in here, and nothing of the library is
launched (consistency_ref64 and the front end's invert_map are host numpy).

Why a twin beside consistency_ref64.warp64.  The restatement sums the four taps in fp64, so a kernel can only be held to it within a
bound (BOUND_WARP of tests/test_consistency_gpu.py), and on smooth images a source position that is 1 / 32 px off stays inside that
bound.  consistency.hip is built with -ffp-contract=off and its header spells every operation out: the positions in fp64, left to
right; then, in fp32, v0 w0 + v1 w1 + v2 w2 + v3 w3, (warped m) / 255, ((m u) 255) / 255, d d, a 2 - 1.  float32 numpy that does ONE
operation per statement, elementwise, is that arithmetic (IEEE multiply, add, divide; no fused multiply-add), so the kernel's RAW
output can be compared bit for bit, on white noise, where a slip of one fixed-point step moves a value by up to 255 / 32.

The block rule (bh0 = min(16, H), bw0 = min(1024 / bh0, W), xb the block's first column) is OpenCV's as the kernel's header and
consistency_ref64.source_positions state it; source_positions_loop below walks it the way WarpPerspectiveInvoker does, block by block,
in Python floats, and shares no indexing with the vectorised rule.
"""
import numpy as np

import consistency_ref64 as R
from pixelsynth_amd import consistency as C

f32 = np.float32
TX, TY = 64, 4                                       # k_consistency_tiles' tile
# c_pnet_shift / c_pnet_scale of csrc/ps_image.h: RGB constants, applied to the BGR-ordered channel j as they stand
PNET_SHIFT = np.array([-0.030, -0.088, -0.188], f32)
PNET_SCALE = np.array([0.458, 0.448, 0.450], f32)
_TAPS = ((0, 0), (1, 0), (0, 1), (1, 1))             # (dx, dy) of tap t = (t & 1, t >> 1)


def block_of(H, W):
    """WarpPerspectiveInvoker's block (bh0, bw0)"""
    bh0 = min(16, H)
    return bh0, min(1024 // bh0, W)


def taps_inside(sx, sy, H, W):
    """-> (4, H, W) bool: tap t of every output pixel lies inside the H x W source"""
    return np.stack([(sx + dx >= 0) & (sx + dx < W) & (sy + dy >= 0) & (sy + dy < H) for dx, dy in _TAPS])


def weights(fx, fy):
    """The four entries of the 32 x 32 bilinear table for the fraction bits (fx, fy), in fp32 (all exact)"""
    tx = (fx.astype(f32) * f32(1.0 / 32.0)).astype(f32)
    ty = (fy.astype(f32) * f32(1.0 / 32.0)).astype(f32)
    ux, uy = (f32(1.0) - tx).astype(f32), (f32(1.0) - ty).astype(f32)
    return [(uy * ux).astype(f32), (uy * tx).astype(f32), (ty * ux).astype(f32), (ty * tx).astype(f32)]


def positions_of(Minv, H, W):
    """consistency_ref64.source_positions, quiet about the NaN and Inf of the saturating maps"""
    with np.errstate(all="ignore"):
        return R.source_positions(Minv, H, W)


def twin32(src_view, ref_view, mask, Minv, positions=None):
    """One direction of k_consistency_tiles: src_view warped by the inverted map Minv (9,) into ref_view's frame, compared under mask.
    Views (3, H, W), mask (1, H, W), each uint8 or fp32 -> (ta, tb, sd, sm): ta, tb (H, W, 3) fp32 BGR as RAW mode writes them
    (t * 2 - 1 of the two compared images), sd = sum m sum_c fl32(d d) and sm = sum m in fp64 (the finish kernel's two sums, which
    it adds in another order).  positions: (sx, sy, fx, fy) in place of positions_of(Minv, H, W), for the sharpness checks.
    Non-finite values go through as IEEE arithmetic has them (NaN * 0 is NaN); a tap outside the image is the literal 0 and is never
    read, so a NaN beside the frame's edge does not reach it."""
    H, W = mask.shape[-2:]
    sx, sy, fx, fy = positions_of(Minv, H, W) if positions is None else positions
    tr = R.try_bgr(src_view)                                             # (H, W, 3): fl32(u * 255)
    w, ok = weights(fx, fy), taps_inside(sx, sy, H, W)
    with np.errstate(all="ignore"):
        warped = None
        for t, (dx, dy) in enumerate(_TAPS):
            v = np.zeros((H, W, 3), f32)
            v[ok[t]] = tr[(sy + dy)[ok[t]], (sx + dx)[ok[t]]]
            p = (v * w[t][..., None]).astype(f32)
            warped = p if warped is None else (warped + p).astype(f32)
        m = R.mask_unit(mask)[..., None]
        a = ((warped * m).astype(f32) / f32(255.0)).astype(f32)
        u = R.unit(ref_view).transpose(1, 2, 0)[:, :, ::-1]
        b = (((m * u).astype(f32) * f32(255.0)).astype(f32) / f32(255.0)).astype(f32)
        d = (a - b).astype(f32)
        dd = (d * d).astype(f32).astype(np.float64)
        d2 = ((0.0 + dd[..., 0]) + dd[..., 1]) + dd[..., 2]
        m64 = m[..., 0].astype(np.float64)
        sd, sm = float((m64 * d2).sum()), float(m64.sum())
        ta = ((a * f32(2.0)).astype(f32) - f32(1.0)).astype(f32)
        tb = ((b * f32(2.0)).astype(f32) - f32(1.0)).astype(f32)
    assert all(x.dtype == f32 for x in (tr, warped, m, a, u, b, d, ta, tb))   # nothing was promoted on the way
    return ta, tb, sd, sm


def standardised(t, j):
    """PS_CONSISTENCY_PERCSIM's value of the BGR-ordered channel j: (t - shift[j]) / scale[j] in fp32"""
    with np.errstate(all="ignore"):
        return ((np.asarray(t, f32) - PNET_SHIFT[j]).astype(f32) / PNET_SCALE[j]).astype(f32)


def psnr64_of(sd, sm):
    """k_consistency_finish's value before its rounding to fp32: 10 log10(1 / (sd / (3 fmax(sm, 1)))) in fp64"""
    den = 3.0 * (sm if sm > 1.0 else 1.0)            # fmax: a NaN sum gives 1 (sd is NaN with it)
    with np.errstate(all="ignore"):
        return float(np.float64(10.0) * np.log10(np.float64(1.0) / (np.float64(sd) / np.float64(den))))


def psnr_of(sd, sm):
    """The finish kernel's output: psnr64_of rounded to fp32, clamped at 100; NaN stays NaN"""
    with np.errstate(all="ignore"):
        p = f32(psnr64_of(sd, sm))
    return f32(100.0) if p > f32(100.0) else p


def ulp_distance(a, b):
    """Between two finite fp32 values of one sign, or 0 for two NaNs or equal values; 2**31 for anything else that differs"""
    a, b = f32(a), f32(b)
    if (np.isnan(a) and np.isnan(b)) or a == b:
        return 0
    if not (np.isfinite(a) and np.isfinite(b)) or (a < 0) != (b < 0):
        return 2 ** 31
    return abs(int(a.view(np.int32)) - int(b.view(np.int32)))


def rounding_is_safe(v64, rel=1e-9):
    """Whether the fp64 value v64 lies further than rel |v64| from both boundaries of its fp32 rounding (the midpoints to the two
    neighbouring fp32 values): then a last-place difference in fp64 cannot change the fp32 result"""
    if not np.isfinite(v64) or not np.isfinite(f32(v64)):
        return True
    f = f32(v64)
    lo = 0.5 * (float(f) + float(np.nextafter(f, f32(-np.inf))))
    hi = 0.5 * (float(f) + float(np.nextafter(f, f32(np.inf))))
    return min(abs(v64 - lo), abs(v64 - hi)) > rel * abs(v64)


def source_positions_loop(Minv, H, W, bw0=None):
    """consistency_ref64.source_positions as OpenCV walks it: per row, per block of bw0 columns, X0 / Y0 / W0 once and then the
    columns of the block, in Python floats.  bw0: another block width than OpenCV's (64, the kernel's tile, is the slip the
    sharpness checks recompute)."""
    M = [float(v) for v in np.asarray(Minv, np.float64).ravel()]
    if bw0 is None:
        bw0 = block_of(H, W)[1]
    hi, lo = float(2 ** 31 - 1), float(-2 ** 31)

    def rnd(v):
        v = v if v < hi else hi                       # std::min(hi, v): NaN -> hi
        v = v if lo < v else lo
        return int(round(v))                          # to nearest, ties to even

    out = np.empty((4, H, W), np.int64)
    for y in range(H):
        for xb in range(0, W, bw0):
            X0 = M[0] * xb + M[1] * y + M[2]
            Y0 = M[3] * xb + M[4] * y + M[5]
            W0 = M[6] * xb + M[7] * y + M[8]
            for x1 in range(min(bw0, W - xb)):
                Wd = W0 + M[6] * x1
                Wd = 32.0 / Wd if Wd != 0.0 else 0.0
                X, Y = rnd((X0 + M[0] * x1) * Wd), rnd((Y0 + M[3] * x1) * Wd)
                out[:, y, xb + x1] = (max(-32768, min(32767, X >> 5)), max(-32768, min(32767, Y >> 5)), X & 31, Y & 31)
    return tuple(out)


# ------------------------------------------------------------------------------------------
# the case table: shapes, maps, views, masks
# ------------------------------------------------------------------------------------------
# the smallest shapes that reach each edge of the kernel (what each reaches: tests/test_consistency_twin_cpu.py asserts it)
SHAPES = [(1, 1), (1, 1100), (3, 7), (5, 300), (12, 200), (15, 70), (17, 65), (37, 130), (130, 37)]
FAMILIES = ("mild", "outside", "saturating")
MASK_KINDS = ("f32", "u8_binary", "u8_bytes")
B = 3
# the saturating family, one map per (item, direction) in this order
SATURATING = ("scale400", "scale1e9", "w_crosses_0", "nan", "inf_w", "neg_inf")
_TRANSPOSED = {(130, 37): (37, 130)}                 # the same data and maps, transposed
_SWAP = [1, 0, 2]


def _seed(H, W, salt):
    return (H * 4099 + W) * 16 + salt


def _framed(Mn, H, W):
    """A map in frame-relative coordinates (the frame is the unit square) -> pixel units: D Mn D^-1, D = diag(W, H, 1)"""
    d = np.array([W, H, 1.0])
    return Mn * d[:, None] / d[None, :]


def tie_map():
    """An affine map whose fixed-point X lies on a rounding tie at every fifth column in exact arithmetic (32 (1.1 x + 0.25 y + 1 / 64)
    = 35.2 x + 8 y + 0.5), so that fp64's last bits decide X there: which way they fall depends on how the sum is split into
    M0 xb and M0 x1, i.e. on the block the column is counted from."""
    return np.array([[1.1, 0.25, 1.0 / 64.0], [0.0, 1.0, 0.25], [0.0, 0.0, 1.0]])


def saturating_map(kind, H, W):
    if kind == "scale400":      # column 0 starts below -32768 px, row 0 just under +32767 px: sat_short acts on both
        return np.array([[400.0, 3.0, -32768.25 - 400.0 * (W // 2)], [5.0, 400.0, 32760.5], [0.0, 0.0, 1.0]])
    if kind == "scale1e9":      # the centre pixel lands on the source's (0, 0), its neighbours beyond int's range; a single column
        cx = W // 2 if W > 1 else 0.5   # or row has no neighbour, so it is sent out itself
        cy = H // 2 if H > 1 else 0.5
        return np.array([[1e9, 0.0, -1e9 * cx], [0.0, 1e9, -1e9 * cy], [0.0, 0.0, 1.0]])
    if kind == "w_crosses_0":   # W = (x - W // 2) / 128: exactly 0 in one column (every term is exact), of either sign beside it
        return np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0], [2.0 ** -7, 0.0, -(W // 2) * 2.0 ** -7]])
    if kind == "nan":
        return np.array([[1.0, 0.0, 0.25], [0.0, np.nan, 0.0], [0.0, 0.0, 1.0]])
    if kind == "inf_w":         # 32 / inf = 0: every pixel reads the source's (0, 0)
        return np.array([[1.0, 0.0, 0.5], [0.0, 1.0, 0.5], [0.0, 0.0, np.inf]])
    if kind == "neg_inf":       # -inf * 0 = NaN in column 0 of each block, -inf after it
        return np.array([[-np.inf, 0.0, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])
    raise KeyError(kind)


def family_maps(H, W, family, n=B):
    """-> (n, 2, 9) fp64: the inverted maps (output pixel -> source position) of n items, direction 0 and 1, as the kernel takes them.
    mild: a projective map within a few percent of the identity in frame-relative coordinates (the bottom row of order 0.1 / W,
    0.1 / H), item 0's direction 0 the tie_map(); outside: scaled by about 1.2 and shifted by up to a quarter of the frame, so part of
    the output comes from outside the source; saturating: SATURATING, through consistency._launch only."""
    if (H, W) in _TRANSPOSED:
        M = family_maps(*_TRANSPOSED[(H, W)], family, n).reshape(n, 2, 3, 3)
        return np.ascontiguousarray(M[:, :, _SWAP][:, :, :, _SWAP].reshape(n, 2, 9))      # P M P, P swapping x and y
    rs = np.random.RandomState(_seed(H, W, FAMILIES.index(family)))
    out = np.empty((n, 2, 3, 3))
    for i in range(n):
        for k in range(2):
            if family == "mild":
                Mn = np.eye(3) + rs.uniform(-1.0, 1.0, (3, 3)) * np.array([[.08, .06, .06], [.06, .08, .06], [.1, .1, 0.0]])
                out[i, k] = tie_map() if (i, k) == (0, 0) else _framed(Mn, H, W)
            elif family == "outside":
                Mn = np.eye(3) + rs.uniform(-1.0, 1.0, (3, 3)) * np.array([[.05, .05, 0.0], [.05, .05, 0.0], [.05, .05, 0.0]])
                for r in range(2):
                    Mn[r, r] += 0.2
                    Mn[r, 2] = -0.25 if rs.randint(2) else 0.08
                out[i, k] = _framed(Mn, H, W)
            else:
                out[i, k] = saturating_map(SATURATING[(2 * i + k) % len(SATURATING)], H, W)
    return np.ascontiguousarray(out.reshape(n, 2, 9))


def views(H, W, dtype, n=B):
    """-> view1, view2 (n, 3, H, W) of white noise: uint8 bytes, or fp32 U(0, 1)"""
    if (H, W) in _TRANSPOSED:
        return tuple(np.ascontiguousarray(v.transpose(0, 1, 3, 2)) for v in views(*_TRANSPOSED[(H, W)], dtype, n))
    if np.dtype(dtype) == np.uint8:
        v = np.random.RandomState(_seed(H, W, 4)).randint(0, 256, (2, n, 3, H, W)).astype(np.uint8)
    else:
        v = np.random.RandomState(_seed(H, W, 5)).rand(2, n, 3, H, W).astype(f32)
    return v[0], v[1]


def masks(H, W, kind, n=B):
    """-> mask1, mask2 (n, 1, H, W): fp32 U(0, 1); uint8 0 / 255; or uint8 of arbitrary bytes (the kernel's table of 256 quotients)"""
    if (H, W) in _TRANSPOSED:
        return tuple(np.ascontiguousarray(m.transpose(0, 1, 3, 2)) for m in masks(*_TRANSPOSED[(H, W)], kind, n))
    rs = np.random.RandomState(_seed(H, W, 6 + MASK_KINDS.index(kind)))
    if kind == "f32":
        m = rs.rand(2, n, 1, H, W).astype(f32)
    elif kind == "u8_binary":
        m = (rs.randint(0, 2, (2, n, 1, H, W)) * 255).astype(np.uint8)
    else:
        m = rs.randint(0, 256, (2, n, 1, H, W)).astype(np.uint8)
    return m[0], m[1]


def directions(view1, view2, mask1, mask2):
    """(src, ref, mask) of direction 0 and 1: view 2 warped into frame 1 under mask 1, then the other way round"""
    return ((view2, view1, mask1), (view1, view2, mask2))


def twin_batch(view1, view2, mask1, mask2, maps):
    """twin32 of every item and direction -> ta, tb (n, 2, H, W, 3) fp32, sums (n, 2, 2) fp64 (sd, sm)"""
    n = len(view1)
    H, W = view1.shape[-2:]
    ta, tb = np.empty((n, 2, H, W, 3), f32), np.empty((n, 2, H, W, 3), f32)
    sums = np.empty((n, 2, 2))
    for i in range(n):
        for k, (src, ref, m) in enumerate(directions(view1, view2, mask1, mask2)):
            ta[i, k], tb[i, k], sums[i, k, 0], sums[i, k, 1] = twin32(src[i], ref[i], m[i], maps[i, k])
    return ta, tb, sums


def forward_of(maps):
    """(n, 2, 9) inverted maps -> H12, H21 (n, 3, 3) for consistency_rows, and the maps its invert_map makes of them again (the
    front end inverts what it is given; direction 0 is H21's)"""
    M = np.asarray(maps).reshape(-1, 2, 3, 3)
    H21, H12 = C.invert_map(M[:, 0]), C.invert_map(M[:, 1])
    back = np.stack([C.invert_map(H21), C.invert_map(H12)], 1).reshape(-1, 2, 9)
    return H12, H21, np.ascontiguousarray(back)
