"""Shared by tests/test_zbuffer_cpu.py and tests/test_zbuffer_gpu.py: a numpy mirror of the two kernels of the hard z-buffer that
DepthManipulator.project_zbuffer runs (pixelsynth_amd/csrc/zbuffer.hip: k_zb_project, and k_zb_test / k_zb_write with an `order`),
and the table of single points the two tests walk.  No test in here, and nothing of the library is imported.

Why a mirror beside oracle/zbuffer_oracle.py.  The oracle multiplies its matrices with `@`, and what BLAS does inside is for BLAS to
say: a product that rounds the other way moves a point on a pixel boundary next door, so a kernel can only be held to the oracle
within a few entries in a thousand.  zbuffer.hip is built with -ffp-contract=off and writes every operation of the projection out,
so float32 numpy that does ONE operation per statement, elementwise, is the kernel's arithmetic and can be compared bit for bit:
RT = RT2 RT1inv as multiplies and adds (load_cams of csrc/splat_math.h), the three matrix-vector products as one multiply and three
fused multiply-adds per row (mat4_vec_fma of zbuffer.hip), ascending k in both.  tests/test_zbuffer_cpu.py holds the mirror itself
against the outputs of the reference's own class (tests/golden/zbuffer.npz) before it judges a kernel.

That the products are fused is the fixture's word.  With multiplies and adds rounded one by one no point changes its pixel or
its flag, but the projected z of 128 000 of the fixture's 524 288 points is a last bit off, the sort order moves at 20 to 186
positions per case, and where two points of one pixel are that close in z the other one stays: 12 sampler entries (8 in demo_small,
4 in mp3d_yaw; none of them among the every-third entries the fixture keeps, all of them in its row sums).  With the fused chain
no entry differs.  For RT the fixture does not tell the two apart: its 4 x 4 products are the same bits either way.

NaN is compared by its bits like everything else.  A quiet NaN that comes in (np.nan, 0x7fc00000) is handed on unchanged, and the
NaN an operation makes out of numbers (0 x inf, inf - inf) is 0xffc00000 on x86, where numpy runs, and on gfx950 alike.
"""
import numpy as np

f32 = np.float32
EPS = f32(1e-2)          # PS_EPS of csrc/splat_math.h (depth_manipulator.py:8)


def fma(a, b, c):
    """fmaf(a, b, c) on float32 arrays, correctly rounded: a b is exact in float64, TwoSum gives the exact error e of the float64 sum s,
    and s is rounded to odd (of the two doubles around s + e the one with the last bit set) before the one rounding to float32 --
    with 29 spare bits that is the rounding of the exact a b + c, where a plain float64 detour rounds twice."""
    p = np.asarray(a, f32).astype(np.float64) * np.asarray(b, f32).astype(np.float64)
    c = np.asarray(c, f32).astype(np.float64)
    with np.errstate(all="ignore"):
        s = p + c
        t = s - p
        e = (p - (s - t)) + (c - t)
        fix = np.isfinite(s) & np.isfinite(e) & (e != 0) & ((np.ascontiguousarray(s).view(np.int64) & 1) == 0)
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(f32)


def _mat4_vec(M, v):
    """k_zb_project's mat4_vec_fma: o[i] = fma(M[i,3], v3, fma(M[i,2], v2, fma(M[i,1], v1, M[i,0] v0))) -- the chain of fused
    multiply-adds, ascending k, that a BLAS sgemm runs for the reference's bmm"""
    out = []
    for i in range(4):
        acc = np.asarray(M[i, 0] * v[0], f32)
        acc = fma(M[i, 1], v[1], acc)
        acc = fma(M[i, 2], v[2], acc)
        acc = fma(M[i, 3], v[3], acc)
        out.append(acc)
    return out


def _mat4_mat4(A, Bm):
    """splat_math.h's load_cams: RT = A Bm per element, ascending k"""
    RT = np.empty((4, 4), f32)
    for i in range(4):
        for j in range(4):
            acc = A[i, 0] * Bm[0, j]
            acc = acc + A[i, 1] * Bm[1, j]
            acc = acc + A[i, 2] * Bm[2, j]
            acc = acc + A[i, 3] * Bm[3, j]
            RT[i, j] = acc
    return RT


def pixel(t):
    """k_zb_project's `pixel`: .long().clamp(0, 255) of the reference (depth_manipulator.py:87-93) without a cast that is undefined.
    Not t > 0 (NaN included) gives 0, t >= 255 gives 255, everything between is truncated towards zero.

    Where this departs from the reference: its .long() of NaN, of +-inf and of a finite |t| >= 2^63 is undefined behaviour; on
    x86 the conversion hands back LONG_MIN for all of them, which the clamp turns into 0.  For NaN, -inf and t <= -2^63 that is
    what stands here too.  For +inf and t >= 2^63 it is not: the kernel saturates them to 255, the side of the image they left
    on, and that is the rule the project keeps (the out-of-range flag is 4 either way)."""
    t = np.asarray(t, f32)
    out = np.zeros(t.shape, np.int32)
    with np.errstate(invalid="ignore"):
        hi = t >= f32(255.0)
        mid = (t > f32(0.0)) & ~hi
    out[hi] = 255
    out[mid] = np.trunc(t[mid]).astype(np.int32)        # 0 < t < 255: the cast is defined
    return out


def project(depth, grid, K, Kinv, RT1inv, RT2):
    """k_zb_project.  depth (B,N), grid (4,N), cameras (B,4,4), all float32 -> zproj (B,N) f32, ys (B,N) i32, xs (B,N) i32,
    flag (B,N) f32, everything by ORIGINAL point position.  zproj is X[2] as the products leave it: the EPS rule replaces the sampler of a
    bad point and never X[2]."""
    depth, grid = np.asarray(depth, f32), np.asarray(grid, f32)
    B, N = depth.shape
    assert grid.shape == (4, N)
    zproj, flag = np.empty((B, N), f32), np.empty((B, N), f32)
    ys, xs = np.empty((B, N), np.int32), np.empty((B, N), np.int32)
    one = np.ones(N, f32)
    with np.errstate(all="ignore"):
        for b in range(B):
            RT = _mat4_mat4(np.asarray(RT2[b], f32), np.asarray(RT1inv[b], f32))
            d = depth[b]
            p = [grid[0] * d, grid[1] * d, grid[2] * d, one]
            c = _mat4_vec(np.asarray(Kinv[b], f32), p)
            w = _mat4_vec(RT, c)
            X = _mat4_vec(np.asarray(K[b], f32), w)
            bad = np.abs(X[2]) < EPS
            sx = X[0] / -X[2]
            sy = X[1] / -X[2]
            sx = np.where(bad, f32(-10.0), sx)
            sy = np.where(bad, f32(-10.0), sy)
            sy = -sy
            tx = (sx + f32(1.0)) * f32(128.0)
            ty = (sy + f32(1.0)) * f32(128.0)
            zproj[b] = X[2]
            xs[b], ys[b] = pixel(tx), pixel(ty)
            flag[b] = np.where((tx < f32(0.0)) | (tx > f32(255.0)) | (ty < f32(0.0)) | (ty > f32(255.0)), f32(4.0), f32(0.0))
    assert all(a.dtype == f32 for a in p + c + w + X + [sx, sy, tx, ty])        # nothing was promoted on the way
    return zproj, ys, xs, flag


def scatter_sorted(order, ys, xs, grid, flag, H, W, out):
    """k_zb_test / k_zb_write with an `order`: the reference's indexed assignment (depth_manipulator.py:95-102) in order, so that
    of several positions on one pixel the LAST stays.  At sorted position n with p = order[b, n]:
        out[b, 0, ys[b, p], xs[b, p]] = grid[0, p] + flag[b, n]        out[b, 1, ...] = -grid[1, p] + flag[b, n]
    (the flag by position n, everything else by point p: the reference's quirk).  A position whose p is outside [0, N) or whose
    pixel is outside the H x W image is skipped; -> whether any was.  `out` (B,2,H,W) is the caller's: what no position hits keeps
    the caller's value.  The assignment is numpy's, which documents that of a repeated index the last value stays;
    scatter_sorted_loop is the same thing one position at a time, and the CPU test holds the two equal."""
    order = np.asarray(order, np.int64)
    B, N = order.shape
    skipped = False
    for b in range(B):
        n = np.nonzero((order[b] >= 0) & (order[b] < N))[0]
        p = order[b, n]
        y, x = ys[b, p], xs[b, p]
        ok = (y >= 0) & (y < H) & (x >= 0) & (x < W)
        skipped |= n.size != N or not ok.all()
        n, p, y, x = n[ok], p[ok], y[ok], x[ok]
        out[b, 0, y, x] = grid[0, p] + flag[b, n]
        out[b, 1, y, x] = -grid[1, p] + flag[b, n]
    return bool(skipped)


def scatter_sorted_loop(order, ys, xs, grid, flag, H, W, out):
    """scatter_sorted, literally: one assignment per sorted position, in order"""
    B, N = order.shape
    skipped = False
    for b in range(B):
        for n in range(N):
            p = int(order[b, n])
            if p < 0 or p >= N or not (0 <= ys[b, p] < H and 0 <= xs[b, p] < W):
                skipped = True
                continue
            out[b, 0, ys[b, p], xs[b, p]] = grid[0, p] + flag[b, n]
            out[b, 1, ys[b, p], xs[b, p]] = -grid[1, p] + flag[b, n]
    return skipped


def project_zbuffer(depth, K, Kinv, RT1inv, RT2, grid):
    """DepthManipulator.project_zbuffer from the two mirrors and a stable argsort of -z (z descending, ties in original order):
    depth (B,1,w,h), grid (4, w*h) -> sampler (B,2,w,h) on a background of -2, projected depth (B,1,w,h), and what project() gave"""
    B, _, w, h = depth.shape
    zproj, ys, xs, flag = project(depth.reshape(B, w * h), grid, K, Kinv, RT1inv, RT2)
    order = np.stack([np.argsort(-zproj[b], kind="stable") for b in range(B)])
    out = np.full((B, 2, w, h), -2.0, f32)
    assert not scatter_sorted(order, ys, xs, grid, flag, w, h, out)
    return out, (-zproj).reshape(B, 1, w, h), (zproj, ys, xs, flag)


# ------------------------------------------------------------------------------------------
# the table of single points
# ------------------------------------------------------------------------------------------
def signed_identity():
    """np.eye(4) in value, with the zeros of row 2 carrying a set sign bit.  Through a plain identity X[2] = +0 p0 + 0 p1 + p2 + 0
    can never be -0.0 (-0 + +0 = +0); through this one every term of row 2 beside p2 is -0.0 for p0, p1 > 0, so a p2 of -0.0 arrives
    as X[2] = -0.0 and the kernel is seen to hand its sign bit on.  (Every other row of the table has |p2| > 0 and is not touched.)"""
    M = np.eye(4, dtype=f32)
    M[2, [0, 1, 3]] = -0.0
    return M


def edge_table():
    """-> rows [(name, g0, g1, g2, d, want)]: one point each, for frame 1 of edge_case() (identity cameras: X = (g0 d, g1 d, g2 d, 1)).
    want is the literal (xs, ys, flag) the point must get, worked out by hand below and not by the mirror, or None.

    With d = 1 and g2 = -1: sx = g0, tx = (g0 + 1) * 128; sy = -g1, ty = (1 - g1) * 128.  g + 1 is exact for every g used (it and
    its sum lie in neighbouring binades with the sum's spacing a multiple of g's), and * 128 is exact, so t is exactly the value
    named.  With u = 2^-23, g + 1 reaches nothing below 0 nearer than -u (floats below -1 are u apart) and nothing beside 255 / 128
    nearer than u, so -2^-16 stands for "the float below 0", and 255 -+ 2^-16 are the floats beside 255 in earnest."""
    u = f32(2.0 ** -23)
    ts = [("t=0", f32(-1.0), 0, 0), ("t=-2^-16, the nearest below 0", f32(-1.0) - u, 0, 4), ("t=-0.5", f32(-1.00390625), 0, 4),
          ("t=254.99998", f32(0.9921875) - u, 254, 0), ("t=255", f32(0.9921875), 255, 0), ("t=255.00002", f32(0.9921875) + u, 255, 4),
          ("t=256", f32(1.0), 255, 4), ("t=1e30", f32(1e30) / f32(128.0), 255, 4), ("t=+inf", f32(3e38), 255, 4)]
    rows = []
    for name, g, px, fl in ts:
        rows.append(("x " + name, g, f32(0.0), f32(-1.0), f32(1.0), (px, 128, fl)))
    for name, g, px, fl in ts:
        rows.append(("y " + name, f32(0.0), -g, f32(-1.0), f32(1.0), (128, px, fl)))
    # EPS rule on X[2] = g2: g0 = g1 = EPS / 2 > 0, so a good point has |sx| = |sy| = 0.5 exactly, and a bad one sx = -10, sy = +10
    h = EPS / f32(2.0)
    good_behind, good_front, bad = (192, 64, 0), (64, 192, 0), (0, 255, 4)
    for name, g2, want in (("-EPS is not bad", -EPS, good_behind), ("nearer zero than -EPS", np.nextafter(-EPS, f32(0.0)), bad),
                           ("+EPS is not bad", EPS, good_front), ("+0.0", f32(0.0), bad), ("-0.0", f32(-0.0), bad),
                           ("1e-30", f32(1e-30), bad)):
        rows.append(("g2 " + name, h, h, g2, f32(1.0), want))
    # depths no scene has: NaN and inf (0 x inf = NaN in the products) land on pixel (0, 0) unflagged, like the reference's; a depth of 0 is a
    # bad point with X[2] = -0.0; a negative depth is a point behind the camera that projects like any other
    q = f32(0.25)
    rows += [("d NaN", q, q, f32(-1.0), f32(np.nan), (0, 0, 0)), ("d +inf", q, q, f32(-1.0), f32(np.inf), (0, 0, 0)),
             ("d 0", q, q, f32(-1.0), f32(0.0), bad), ("d -2", q, q, f32(-1.0), f32(-2.0), (160, 96, 0))]
    return rows


def edge_case(seed=0):
    """The table as a call of ps_zbuffer_project_f32: B = 2, W = 6 (N = 36: the table and padding).  Frame 1 has signed_identity()
    for all four cameras; frame 0 has random ones, so that a kernel that reads frame 0's cameras for every frame fails frame 1's
    literals.  -> dict(W, depth (2,N), grid (4,N), K, Kinv, RT1inv, RT2 (2,4,4), rows)"""
    rows = edge_table()
    W = 6
    N = W * W
    assert len(rows) <= N
    rs = np.random.RandomState(seed)
    grid = np.zeros((4, N), f32)
    grid[2], grid[3] = -1.0, 1.0
    depth = np.ones((2, N), f32)
    for i, (_, g0, g1, g2, d, _) in enumerate(rows):
        grid[:3, i] = g0, g1, g2
        depth[:, i] = d
    grid[:2, len(rows):] = rs.uniform(-0.9, 0.9, size=(2, N - len(rows)))        # padding: ordinary points
    cams = [np.stack([(np.eye(4) + 0.3 * rs.randn(4, 4)).astype(f32), signed_identity()]) for _ in range(4)]
    return dict(W=W, depth=depth, grid=grid, K=cams[0], Kinv=cams[1], RT1inv=cams[2], RT2=cams[3], rows=rows)
