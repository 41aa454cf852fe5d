"""CPU: the NumPy definition of Pareto-smoothed importance sampling and of the pointwise PSIS-LOO / WAIC estimates
(mcmc_spec_amd/psis.py), which tests/test_gpu_psis.py holds the device to.  No GPU."""
import numpy as np
import pytest

import common  # noqa: F401
from mcmc_spec_amd import psis


def pareto_ratios(k, S=20000, seed=3):
    """Log-ratios whose weights exp(lr) follow a Pareto law of shape k: lr = k * Exponential(1)."""
    return k * np.random.default_rng(seed).exponential(1.0, S)


def test_tail_len_is_the_papers_expression():
    assert psis.tail_len(20000) == 425 and psis.tail_len(24) == 5 and psis.tail_len(100) == 20 and psis.tail_len(2) == 1
    assert psis.tail_len(20000, reff=0.25) == int(np.ceil(3.0 * np.sqrt(80000.0)))
    assert list(psis.tail_len(np.array([24, 1000]))) == [5, 95]
    assert psis.LOG_TINY == float(np.log(np.finfo(np.float64).tiny))


def test_khat_orders_with_the_pareto_shape():
    khat = [psis.smooth(pareto_ratios(k), psis.tail_len(20000))['khat'] for k in (0.2, 0.5, 0.9)]
    print('khat for k = 0.2, 0.5, 0.9:', khat)
    assert khat[0] < khat[1] < khat[2]
    assert khat[0] < 0.5 and khat[2] > 0.7


@pytest.mark.parametrize('k', [0.2, 0.5, 0.9])
def test_the_smoothed_weights_are_normalised_monotone_and_touch_the_tail_alone(k):
    lr = pareto_ratios(k, seed=11)
    M = psis.tail_len(lr.size)
    r = psis.smooth(lr, M)
    assert r['status'] == psis.OK and r['S'] == lr.size and r['tail'].size == M
    assert abs(psis.logsumexp(r['lw'])) <= 1e-12
    tail = r['tail']
    # the tail is the M largest, in ascending order of (value, index)
    assert np.array_equal(tail, np.argsort(lr, kind='stable')[-M:])
    smoothed = r['pre'][tail]
    assert np.all(np.diff(smoothed) >= 0.0) and np.all(smoothed <= 0.0)
    rest = np.ones(lr.size, dtype=bool)
    rest[tail] = False
    assert np.array_equal(r['pre'][rest], (lr - lr.max())[rest])
    assert np.all(r['pre'][rest] <= r['cutoff']) and np.all((lr - lr.max())[tail] > r['cutoff'])
    # the normalisation is one subtraction
    assert np.array_equal(r['lw'], r['pre'] - psis.logsumexp(r['pre']))


def test_a_tail_of_four_is_short_and_a_tail_of_five_is_fitted():
    rng = np.random.default_rng(3)
    lr = rng.normal(0.0, 1.0, 24)
    four, five = psis.smooth(lr, 4), psis.smooth(lr, 5)
    assert four['status'] == psis.SHORT_TAIL and four['khat'] == np.inf and four['tail'].size == 4
    assert np.array_equal(four['pre'], lr - lr.max())                  # nothing is smoothed
    assert abs(psis.logsumexp(four['lw'])) <= 1e-12
    assert five['status'] == psis.OK and np.isfinite(five['khat']) and five['tail'].size == 5
    # constant log-ratios: nothing lies strictly above the cutoff
    flat = psis.smooth(np.full(50, -3.25), psis.tail_len(50))
    assert flat['status'] == psis.SHORT_TAIL and flat['khat'] == np.inf and flat['tail'].size == 0
    assert np.array_equal(flat['lw'], np.full(50, -np.log(50.0)))
    for bad_len in (0, 24, 50):
        with pytest.raises(ValueError):
            psis.smooth(lr, bad_len)


def test_ties_across_the_cutoff_shorten_the_tail_deterministically():
    lr = np.arange(40, dtype=np.float64) * 0.25
    lr[28:33] = lr[30]               # five equal values; the cutoff (rank 40 - 8 - 1 = 31) falls among them
    r = psis.smooth(lr, 8)
    assert list(r['tail']) == [33, 34, 35, 36, 37, 38, 39] and r['status'] == psis.OK
    # equal values inside the tail keep index order
    lr2 = np.concatenate([np.zeros(30), [1.0, 2.0, 2.0, 2.0, 3.0, 3.0, 4.0]])[::-1].copy()
    r2 = psis.smooth(lr2, 7)
    assert list(r2['tail']) == [6, 3, 4, 5, 1, 2, 0]
    assert np.all(np.diff(r2['pre'][r2['tail']]) >= 0.0)


def test_bad_and_minus_infinite_entries_weigh_nothing():
    lr = pareto_ratios(0.4, S=400, seed=2)
    lr[[3, 77]] = np.nan
    lr[[5, 200]] = np.inf
    lr[[9, 10, 11]] = -np.inf
    r = psis.smooth(lr, psis.tail_len(396))
    assert r['S'] == 396 and r['status'] == psis.OK
    assert np.all(r['lw'][[3, 77, 5, 200, 9, 10, 11]] == -np.inf) and np.all(np.isfinite(np.delete(r['lw'], [3, 77, 5, 200, 9, 10, 11])))
    assert abs(psis.logsumexp(r['lw'])) <= 1e-12
    clean = psis.smooth(np.delete(lr, [3, 77, 5, 200]), psis.tail_len(396))   # the bad entries do not count; -inf does
    assert clean['khat'] == r['khat'] and np.array_equal(clean['lw'], np.delete(r['lw'], [3, 77, 5, 200]))
    s = psis.series_weights(lr.reshape(100, 4), [psis.tail_len(198)] * 2, counts=[2, 2])
    assert np.all(s['w'].reshape(-1)[[3, 77, 5, 200, 9, 10, 11]] == 0.0) and s['w'].max() == 1.0
    assert list(s['stats']['nbad']) == [int(np.sum(~np.isfinite(lr.reshape(100, 4)[:, :2]) & ~(lr.reshape(100, 4)[:, :2] == -np.inf))),
                                        int(np.sum(~np.isfinite(lr.reshape(100, 4)[:, 2:]) & ~(lr.reshape(100, 4)[:, 2:] == -np.inf)))]
    nothing = psis.smooth(np.array([-np.inf, -np.inf, np.nan, -np.inf]), 1)
    assert nothing['status'] == psis.SHORT_TAIL and np.all(nothing['lw'] == -np.inf)


def test_pointwise_stats_and_compare():
    rng = np.random.default_rng(8)
    y = rng.normal(0.0, 1.0, 12)
    mu_a, mu_b = rng.normal(0.0, 0.3, 300), rng.normal(0.5, 0.3, 300)
    ll = lambda mu: -0.5 * (y[:, None] - mu[None, :]) ** 2 - 0.5 * np.log(2.0 * np.pi)
    a, b = psis.pointwise_stats(ll(mu_a)), psis.pointwise_stats(ll(mu_b))
    for r in (a, b):
        assert r['n_obs'] == 12 and np.all(r['p_waic'] >= 0.0) and np.all(np.isfinite(r['khat']))
        for name in ('lppd', 'p_waic', 'elpd_waic', 'elpd_loo', 'p_loo'):
            assert r['total'][name] == float(np.sum(r[name]))
            assert r['se'][name] == float(np.sqrt(12 * np.var(r[name], ddof=1)))
        assert np.array_equal(r['elpd_waic'], r['lppd'] - r['p_waic']) and np.array_equal(r['p_loo'], r['lppd'] - r['elpd_loo'])
        assert np.all(r['elpd_loo'] <= r['lppd'] + 1e-12)              # leaving an observation out never helps predicting it
        assert r['n_bad_k'] == int(np.sum(r['khat'] > 0.7))
        assert np.allclose(r['p_waic'], np.var(ll(mu_a if r is a else mu_b), axis=1, ddof=1), rtol=1e-12)
    assert a['total']['elpd_loo'] > b['total']['elpd_loo']               # the model centred on the data predicts better
    ab, ba = psis.compare(a, b), psis.compare(b, a)
    for name in ('elpd_loo', 'elpd_waic'):
        assert ab[name][0] == -ba[name][0] and ab[name][1] == ba[name][1] and ab[name][1] > 0.0
        assert ab[name][0] == pytest.approx(a['total'][name] - b['total'][name], rel=1e-12)
    with pytest.raises(ValueError):
        psis.compare(a, psis.pointwise_stats(ll(mu_a)[:5]))
