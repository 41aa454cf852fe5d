"""CPU: the NumPy definition of importance reweighting (mcmc_spec_amd/reweight.py) against plain
NumPy where plain NumPy is exact -- weights that are multiples of 2^-10 with sums below 2^40 make every prefix sum exact,
whatever the order -- and against hand-computed cases."""
import numpy as np
import pytest

import common  # noqa: F401
from mcmc_spec_amd import reweight as rw

T = rw.TILE


def dyadic(n, seed, zeros=0.2):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 14, size=n).astype(np.float64) / 1024.0
    w[rng.random(n) < zeros] = 0.0
    return w


@pytest.mark.parametrize('n', [1, 2, 255, 256, 257, T - 1, T, T + 1, 2 * T + 3, 5 * T + 77])
def test_prefix_sums_of_dyadic_weights_are_numpys_cumsum(n):
    w = dyadic(n, n)
    w[-1] = 3.5   # (the last sample weighs)
    C = rw.prefix_sums(w)
    assert C.shape == (n,) and np.array_equal(C, np.cumsum(w)) and C[-1] < 2.0 ** 40
    assert np.all(np.diff(C) >= 0.0)


@pytest.mark.parametrize('n,nout', [(1, 1), (1, 5), (2, 3), (T - 1, 700), (T, T), (T + 1, 2 * T), (2 * T + 3, 999), (5 * T + 77, 10 * T)])
def test_drawn_indices_of_dyadic_weights_are_numpys_searchsorted(n, nout):
    w = dyadic(n, 100 + n)
    w[0] = 1.0
    for u in (0.0, 0.25, 0.9990234375):
        idx = rw.draw(w, nout, u)
        c = np.cumsum(w)
        t = (np.arange(nout) + u) * (c[-1] / nout)
        want = np.minimum(np.searchsorted(c, t, side='right'), np.nonzero(w > 0)[0][-1])
        assert idx.dtype == np.int64 and np.array_equal(idx, want)
        assert np.all(w[idx] > 0.0) and np.all(np.diff(idx) >= 0)


def test_general_weights_give_a_scan_that_never_decreases_and_stays_near_cumsum():
    """Both serial levels of the scan make C monotone in floating point: searchsorted is then the first i with C_i > t."""
    rng = np.random.default_rng(5)
    w = np.exp(rng.normal(0.0, 3.0, size=7 * T + 13))
    C = rw.prefix_sums(w)
    assert np.all(np.diff(C) >= 0.0)
    assert np.allclose(C, np.cumsum(w), rtol=1e-12, atol=0.0)
    idx = rw.draw(w, 4000, 0.5)
    t = (np.arange(4000) + 0.5) * (C[-1] / 4000)
    first = np.array([np.argmax(C > x) if np.any(C > x) else len(C) - 1 for x in t[::97]])
    assert np.array_equal(idx[::97], first)


def test_hand_computed_cases():
    # N = 1: every draw is sample 0
    assert np.array_equal(rw.draw([0.37], 4, 0.6), [0, 0, 0, 0])
    # all weight on one sample
    w = np.zeros(300)
    w[117] = 2.0
    assert np.array_equal(rw.draw(w, 9, 0.1), np.full(9, 117))
    # ... on the last one: C_{N-1} > t_j fails for no j, and a t_j that rounds up to W is clamped
    w = np.zeros(T + 5)
    w[-1] = 1.0
    assert np.array_equal(rw.draw(w, 7, 0.999999), np.full(7, T + 4))
    # equal weights, nout = N: 0 .. N - 1 in order, wherever the comb starts
    for n in (1, 5, 256, T + 1):
        for u in (0.0, 0.5, 0.999):
            assert np.array_equal(rw.draw(np.ones(n), n, u), np.arange(n))
    # weights 1, 0, 3 and four draws at u = 0.5: t = 0.5, 1.5, 2.5, 3.5 against C = 1, 1, 4
    assert np.array_equal(rw.draw([1.0, 0.0, 3.0], 4, 0.5), [0, 2, 2, 2])
    # trailing zero weights are never drawn: t = 0.75, 1.75 against C = 1, 2, 2, 2
    assert np.array_equal(rw.draw([1.0, 1.0, 0.0, 0.0], 2, 0.75), [0, 1])
    with pytest.raises(ValueError):
        rw.draw(np.zeros(4), 2, 0.5)
    with pytest.raises(ValueError):
        rw.draw([1.0, -1.0, 3.0], 2, 0.5)


def test_u0_is_the_counter_generators_stream_15():
    from mcmc_spec_amd.sampler import counter_streams
    a, b = rw.u0(7, 0), rw.u0(7, 1)
    assert 0.0 <= a < 1.0 and 0.0 <= b < 1.0 and a != b and rw.u0(8, 0) != a
    assert a == counter_streams(7, 0, 1, 4)[2](15, 3)[0, 0] and rw.u0(7, 0) == a
    # SplitMix64's output function of seed * K + (ctr + 1) * gamma, ctr = (member << 28) + (15 << 24)
    mask = (1 << 64) - 1
    x = (7 * 0xD1342543DE82EF95 + (((1 << 28) + (15 << 24)) + 1) * 0x9E3779B97F4A7C15) & mask
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & mask
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & mask
    x ^= x >> 31
    assert b == (x >> 11) / 9007199254740992.0


def test_weighted_mean_of_dyadic_data_is_numpys_average():
    """Dyadic weights and dyadic data: every product and partial sum is exact, so the fixed order gives np.average's sums and
    the two results differ by the one division's rounding at most -- here by nothing."""
    rng = np.random.default_rng(11)
    counts = [2, 3]
    x = rng.integers(-(1 << 12), 1 << 12, size=(700, 5, 3)).astype(np.float64) / 64.0
    w = rng.integers(0, 1 << 10, size=(700, 5)).astype(np.float64) / 1024.0
    for discard, thin in ((0, 1), (13, 3)):
        got = rw.wmoments(x, w, counts, discard, thin, cols=[2, 0])
        xs, ws = rw.flat(x, counts, discard, thin), rw.flat(w, counts, discard, thin)
        for m in range(2):
            assert got['sumw'][m] == ws[m].sum()
            assert np.array_equal(got['mean'][m], [np.sum(ws[m] * xs[m][:, c]) / ws[m].sum() for c in (2, 0)])
            assert np.allclose(got['mean'][m], np.average(xs[m][:, [2, 0]], axis=0, weights=ws[m]), rtol=4e-16, atol=0.0)
            assert np.allclose(got['cov'][m], np.cov(xs[m][:, [2, 0]].T, aweights=ws[m], ddof=0), rtol=1e-12, atol=0.0)
            assert np.array_equal(got['cov'][m], got['cov'][m].T)


def test_weights_and_their_statistics():
    rng = np.random.default_rng(3)
    counts = [2, 3]
    logw = rng.normal(0.0, 2.0, size=(90, 5))
    logw[4, 0], logw[5, 1], logw[6, 3], logw[7, 4] = np.nan, np.inf, -np.inf, np.nan
    w = rw.weights(logw, counts)
    M = rw.member_max(logw, counts)
    assert M[0] == np.nanmax(np.where(np.isinf(logw[:, :2]), np.nan, logw[:, :2]))
    assert w[4, 0] == w[5, 1] == w[6, 3] == w[7, 4] == 0.0 and w.max() == 1.0 and np.all(w >= 0.0)
    st = rw.weight_stats(logw, w, counts)
    assert list(st['count']) == [180, 270] and list(st['nbad']) == [2, 1] and list(st['nzero']) == [0, 1]
    assert np.allclose(st['sumw'], [w[:, :2].sum(), w[:, 2:].sum()], rtol=1e-13)
    assert np.allclose(st['ess'], st['sumw'] ** 2 / st['sumw2']) and np.all((st['ess'] > 1.0) & (st['ess'] < st['count']))
    # a member without a finite value: every weight 0, ESS 0
    logw[:, 2:] = -np.inf
    logw[3, 2] = np.nan
    w = rw.weights(logw, counts)
    st = rw.weight_stats(logw, w, counts, discard=1, thin=2)
    assert np.all(w[:, 2:] == 0.0) and st['ess'][1] == 0.0 and st['sumw'][1] == 0.0 and st['nbad'][1] == 1 and st['nzero'][1] == 45 * 3 - 1
    # equal log-weights: ESS = N exactly
    st = rw.weight_stats(np.zeros((64, 5)), rw.weights(np.zeros((64, 5)), counts), counts)
    assert list(st['ess']) == [128.0, 192.0]


def test_lincomb_is_numpys_expression_and_a_zero_weight_enters_no_sum():
    rng = np.random.default_rng(8)
    a, b, c = rng.normal(size=(3, 40, 5))
    assert np.array_equal(rw.lincomb([(a, 1.0), (b, -1.0)]), 1.0 * a + -1.0 * b)
    assert np.array_equal(rw.lincomb([(a, 0.3), (b, -0.7), (c, 1e-3)]), 0.3 * a + -0.7 * b + 1e-3 * c)
    x = rng.normal(size=(40, 5, 2))
    w = rng.random((40, 5))
    w[3, 1] = 0.0
    x[3, 1, 0] = np.nan
    clean = rw.wmoments(x, w, [5])
    assert np.all(np.isfinite(clean['mean'])) and np.all(np.isfinite(clean['cov']))
    w[3, 1] = 0.5   # with a weight the value poisons its column, and only its column
    bad = rw.wmoments(x, w, [5])
    assert np.isnan(bad['mean'][0, 0]) and np.isfinite(bad['mean'][0, 1]) and np.isfinite(bad['cov'][0, 1, 1]) and np.isnan(bad['cov'][0, 0, 1])


def test_resample_returns_the_drawn_rows_of_every_member():
    rng = np.random.default_rng(2)
    x = rng.normal(size=(50, 5, 4))
    w = rng.random((50, 5))
    out, idx = rw.resample(x, w, [30, 0], seed=9, counts=[2, 3], discard=4, thin=2)
    xs = rw.flat(x, [2, 3], 4, 2)
    assert out[0].shape == (30, 4) and out[1].shape == (0, 4) and np.array_equal(out[0], xs[0][idx[0]])
    assert np.array_equal(idx[0], rw.draw(rw.flat(w, [2, 3], 4, 2)[0], 30, rw.u0(9, 0)))
