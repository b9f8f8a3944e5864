"""CPU-only: the oracle of the nearest-code kernel (oracle/pixelsynth_oracle.c: ps_oracle_vq_nearest, the definition of
ps_vq_nearest_f32 in include/pixelsynth_hip.h restated in plain C) against float64 distances, and its rule at exact ties and at rows
or codebook columns that are not finite.  tests/test_vq_nearest_gpu.py then holds the kernel to this oracle bit for bit.

The rounding bound.  zz, ee and dot are chains of D fused multiply-adds, each step rounding once (relative 2^-24 of a partial sum that
the sum of the terms' magnitudes bounds), and two additions follow, so with d64 the float64 distance
    |dist - d64| <= (D + 3) 2^-24 (sum z^2 + 2 sum |z_d e_dk| + sum e^2) =: bound[n, k]
(to first order; (D + 3) for D + 2 leaves room for the second-order terms and for float64's own rounding of d64)."""
import numpy as np
import pytest

import _vq_nearest_cases as cases
from oracle import c_oracle


def fp64_distances(z, emb):
    """-> d64 (N, K), bound (N, K)"""
    z, emb = z.astype(np.float64), emb.astype(np.float64)
    zz, ee = (z * z).sum(1, keepdims=True), (emb * emb).sum(0, keepdims=True)
    d64 = zz - 2.0 * (z @ emb) + ee
    bound = (z.shape[1] + 3) * 2.0 ** -24 * (zz + 2.0 * (np.abs(z) @ np.abs(emb)) + ee)
    return d64, bound


@pytest.mark.parametrize("N,D,K", cases.SHAPES)
def test_oracle_against_fp64(N, D, K):
    z, emb = cases.random_case(N, D, K)
    idx, md = c_oracle.vq_nearest(z, emb)
    assert idx.dtype == np.int32 and md.dtype == np.float32 and idx.shape == md.shape == (N,)
    assert idx.min() >= 0 and idx.max() < K
    d64, bound = fp64_distances(z, emb)
    rows, best = np.arange(N), d64.argmin(1)
    err = np.abs(md.astype(np.float64) - d64[rows, idx])
    ratio = float((err / bound[rows, idx]).max())
    if K > 1:
        two = np.partition(d64, 1, axis=1)[:, :2]
        decided = (two[:, 1] - two[:, 0]) > 2.0 * bound.max(1)
    else:
        decided = np.ones(N, bool)
    print(f"vq_nearest oracle N={N} D={D} K={K}: max |mindist - d64| / bound = {ratio:.3f}, rows decided {decided.mean():.4f}")
    assert np.all(err <= bound[rows, idx])
    assert np.all(d64[rows, idx] <= d64[rows, best] + bound[rows, idx] + bound[rows, best])
    assert np.array_equal(idx[decided], best[decided])
    assert decided.mean() >= 0.99


def test_oracle_exact_ties_take_the_smaller_index():
    z, emb, want = cases.tie_case()
    idx, md = c_oracle.vq_nearest(z, emb)
    assert np.array_equal(idx, want)
    assert np.array_equal(cases.bits(md), np.zeros(len(want), np.int32))     # +0.0
    z, emb = cases.identical_columns_case()
    idx, _ = c_oracle.vq_nearest(z, emb)
    assert np.array_equal(idx, np.zeros(len(z), np.int32))


def test_oracle_hostile_rows_give_code_0_and_leave_the_others_alone():
    z, clean, emb = cases.hostile_case()
    idx, md = c_oracle.vq_nearest(z, emb)
    assert idx.min() >= 0 and idx.max() < emb.shape[1]
    bad = list(cases.HOSTILE_ROWS)
    assert np.array_equal(idx[bad], np.zeros(len(bad), np.int32))
    assert np.all(np.isposinf(md[bad]))
    idx0, md0 = c_oracle.vq_nearest(clean, emb)
    good = np.setdiff1d(np.arange(len(z)), bad)
    assert np.array_equal(idx[good], idx0[good]) and np.array_equal(cases.bits(md[good]), cases.bits(md0[good]))
    assert np.all(np.isfinite(md[good]))


def test_oracle_never_chooses_a_column_that_is_not_finite():
    z, emb = cases.hostile_codebook_case()
    idx, md = c_oracle.vq_nearest(z, emb)
    assert not np.isin(idx, cases.BAD_COLUMNS).any() and np.all(np.isfinite(md))
    keep = np.setdiff1d(np.arange(emb.shape[1]), cases.BAD_COLUMNS)
    idx1, md1 = c_oracle.vq_nearest(z, np.ascontiguousarray(emb[:, keep]))   # the same codebook without the two columns
    assert np.array_equal(keep[idx1], idx) and np.array_equal(cases.bits(md1), cases.bits(md))


def test_layout_helper_is_the_headers_row_order():
    """to_layout1: row n = b * HW + p of the (N, D) array is [b, :, p] of the (B, D, HW) one (include/pixelsynth_hip.h)."""
    z = np.arange(3 * 7 * 5, dtype=np.float32).reshape(21, 5)
    t = cases.to_layout1(z, 3, 7)
    assert t.shape == (3, 5, 7)
    for n in (0, 6, 7, 20):
        assert np.array_equal(t[n // 7, :, n % 7], z[n])
