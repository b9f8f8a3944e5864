"""The fp64 reference of the fused categorical draw (oracle/lmconv_oracle.py: draw_distribution, inverse_cdf), which the
GPU tests of csrc/lmconv_device.h:draw_code rely on, checked on distributions whose inverse CDF is known exactly."""
import numpy as np

from oracle import lmconv_oracle as lo


def test_inverse_cdf_of_equal_classes_is_floor_512u():
    p, pos = lo.draw_distribution(np.zeros(512, np.float32), 0.7)
    assert pos.all() and np.allclose(p, 1 / 512)
    u = np.concatenate([np.arange(512) / 512, np.random.RandomState(0).rand(1000), [1 - 2.0 ** -24, 2.0 ** -24]])
    k, _ = lo.inverse_cdf(p, u)
    np.testing.assert_array_equal(k, np.floor(u * 512).astype(np.int64))


def test_zero_classes_are_zero_in_both_precisions_and_never_drawn():
    lg = np.random.RandomState(1).uniform(-1.5, 0, 512).astype(np.float32)
    lg[0], lg[200:], lg[[7, 8, 15, 16]] = 0.0, -6000.0, -6000.0
    for T in (0.05, 0.7, 1.0, 5.0):
        p, pos = lo.draw_distribution(lg, T)
        np.testing.assert_array_equal(p > 0, pos)
        assert pos.sum() == 200 - 4 and not pos[200:].any()
        u = np.concatenate([np.random.RandomState(2).rand(20000), [0.0, 2.0 ** -24, 1 - 3 * 2.0 ** -24, 1 - 2.0 ** -23, 1 - 2.0 ** -24]])
        k, acc = lo.inverse_cdf(p, u, edge=2.0 ** -20)
        assert pos[k].all() and k[-1] == 199 and k[-5] == 0
        assert not acc[:, ~pos].any()                       # the slack never admits a class of probability 0
        cdf = np.cumsum(p) / p.sum()
        assert ((cdf[k] > u) & (np.where(k > 0, cdf[k - 1], 0) <= u)).all()


def test_underflow_through_the_temperature():
    """Natural logits at a low temperature: fp32 exp underflows in the tail, fp64 does not."""
    lg = (np.random.RandomState(3).randn(512) * 3).astype(np.float32)
    p, pos = lo.draw_distribution(lg, 0.05)
    assert (p > 0).all() and 0 < pos.sum() < 512
    x = lg / np.float32(0.05)
    assert (x[~pos] - x.max() < -87).all()


def test_edge_slack_admits_the_neighbour_across_an_edge_only():
    lg = np.full(512, -6000.0, np.float32)
    lg[[100, 401]] = 0.0                                    # two tied classes: the edge is at 1/2
    p, _ = lo.draw_distribution(lg, 1.0)
    k, acc = lo.inverse_cdf(p, np.array([0.25, 0.5 - 2.0 ** -22, 0.5, 0.75]), edge=2.0 ** -20)
    np.testing.assert_array_equal(k, [100, 100, 401, 401])
    np.testing.assert_array_equal(acc.sum(1), [1, 2, 2, 1])
    assert acc[1, 401] and acc[2, 100]


def test_quantile_grid_counts_match_n_p():
    lg = np.random.RandomState(4).uniform(-1.5, 0, 512).astype(np.float32)
    lg[300:] = -6000.0
    p, _ = lo.draw_distribution(lg, 0.05)
    n = 4096
    k, _ = lo.inverse_cdf(p, (np.arange(n) + 0.5) / n)
    assert np.abs(np.bincount(k, minlength=512) - n * p).max() <= 1
