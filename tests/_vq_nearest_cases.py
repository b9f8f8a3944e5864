"""Inputs the nearest-code tests share (tests/test_vq_nearest_cpu.py on the oracle alone, tests/test_vq_nearest_gpu.py on the kernel):
the random shapes, the exact ties and the hostile rows.  Plain numpy; nothing here touches a device."""
import numpy as np

# (N, D, K).  k_vq_nearest (csrc/vq.hip): 16 rows per workgroup, 256 threads striding over K, four waves of 64.
SHAPES = [(1, 1, 1), (17, 64, 512), (37, 8, 5), (300, 33, 700), (48, 64, 257), (50, 3, 1025), (1000, 64, 512)]


def random_case(N, D, K):
    rs = np.random.RandomState(1000003 * N + 1009 * D + K)
    return rs.randn(N, D).astype(np.float32), rs.randn(D, K).astype(np.float32)


# Column b is a copy of column a; row i of z is column a_i, so both are at distance exactly 0.0 (zz, ee and dot are the same chain)
# and every other column is further.  Where the two candidates meet in k_vq_nearest (thread t = k % 256, lane t % 64, wave t / 64):
TIE_PAIRS = [
    (3, 5),        # lanes 3 and 5 of wave 0: the shuffle merge inside one wave
    (10, 70),      # lane 10 of wave 0, lane 6 of wave 1: the merge across waves through LDS
    (100, 356),    # both are thread 100's (k and k + 256): the strict < of the scan
    (255, 256),    # lane 63 of wave 3 against lane 0 of wave 0: the smaller k sits in the HIGHER wave
    (511, 512),    # thread 255's second code against thread 0's third: the same, one stride up
    (0, 699),      # the first and the last column
]
TIE_D, TIE_K = 64, 700


def tie_case():
    """-> z (6, 64), embed (64, 700), want (6,) int32"""
    rs = np.random.RandomState(77)
    emb = rs.randn(TIE_D, TIE_K).astype(np.float32)
    for a, b in TIE_PAIRS:
        emb[:, b] = emb[:, a]
    a = np.array([p[0] for p in TIE_PAIRS])
    return np.ascontiguousarray(emb[:, a].T), emb, a.astype(np.int32)


def identical_columns_case(N=20):
    """Every column the same vector: all K distances of a row are equal bit for bit -> 0."""
    rs = np.random.RandomState(78)
    col = rs.randn(TIE_D, 1).astype(np.float32)
    return rs.randn(N, TIE_D).astype(np.float32), np.ascontiguousarray(np.repeat(col, TIE_K, 1))


HOSTILE_ROWS = (5, 17, 18, 20, 33)


def hostile_case():
    """-> z (48, 64) with the rows of HOSTILE_ROWS hostile, the same with those rows zeroed, embed (64, 512).  Three workgroups."""
    rs = np.random.RandomState(79)
    z, emb = rs.randn(48, 64).astype(np.float32), rs.randn(64, 512).astype(np.float32)
    z[5, 11] = np.nan                  # every dot and zz of the row are NaN
    z[17, 3] = np.inf                  # zz = +inf, dot = +-inf: inf - inf
    z[18, 60] = -np.inf
    z[20, :] = 1e30                    # zz overflows at its first step
    z[33, :] = 1e19                    # zz = 64e38 overflows while every dot stays finite: dist = +inf for every k, never < +inf
    clean = z.copy()
    clean[list(HOSTILE_ROWS)] = 0.0
    return z, clean, emb


BAD_COLUMNS = (7, 300)


def hostile_codebook_case():
    """A finite z against a codebook whose column 7 is all NaN and column 300 all +inf: neither may be chosen."""
    rs = np.random.RandomState(80)
    z, emb = rs.randn(48, 64).astype(np.float32), rs.randn(64, 512).astype(np.float32)
    emb[:, 7] = np.nan
    emb[:, 300] = np.inf
    return z, emb


def to_layout1(z, B, HW):
    """(B * HW, D) rows -> the (B, D, HW) array whose row b * HW + p they are"""
    return np.ascontiguousarray(z.reshape(B, HW, -1).transpose(0, 2, 1))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)
