"""CPU: rank-normalised R-hat, bulk / tail ESS and MCSE on the host (mcmc_spec_amd.diagnostics) against
the loops of tests/rank_numpy.py; ranks and ndtri against SciPy; the NaN rules; what the classic split R-hat misses; AR(1) and
Metropolis-like repeats; the protocols' ``ess=``; the host group and ladder samplers."""
import os

import numpy as np
import pytest
import scipy.special
import scipy.stats

import common  # noqa: F401
import rank_numpy as rn
from mcmc_spec_amd import diagnostics
from mcmc_spec_amd.group import GroupSampler, run_group_protocol
from mcmc_spec_amd.sampler import EnsembleSampler, run_reference_protocol
from mcmc_spec_amd.tempered import TemperedSampler

Q = (0.16, 0.5, 0.84)


def data(n, W, seed):
    """(n, W, 3): a wide column away from zero, a narrow one, a heavy-tailed one."""
    rng = np.random.default_rng(seed)
    return np.stack([rng.normal(-300.0, 40.0, (n, W)), rng.normal(5.0, 1.0, (n, W)), rng.standard_cauchy((n, W))], axis=2)


def definition(x, counts=None):
    out = dict(diagnostics.rank_rhat(x, counts))
    for kind in ('bulk', 'tail', 'mean'):
        out['ess_' + kind] = diagnostics.ess(x, kind, counts)
    m = diagnostics.mcse(x, Q, counts)
    out['mcse_mean'], out['mcse_quantile'] = m['mean'], m['quantiles']
    out['ess_quantile'] = np.stack([diagnostics.ess_quantile(x, p, counts) for p in Q], axis=-1)
    return out


# The loops sum with fsum; the definition with NumPy's pairwise sums and an FFT autocovariance whose absolute error is a few
# 1e-16 A(0).  The pair sums that end Geyer's sequence are checked to be away from zero, so both cut at the same lag; tau is
# then a sum of at most h terms of size <= 1 and >= 1 / log10(S) >= 0.2: 1e-10 relative leaves four orders.
@pytest.mark.parametrize('n', [4, 5, 11])
def test_the_definition_against_written_out_loops(n):
    x, counts, off = data(n, 18, n), [4, 8, 6], [0, 4, 12, 18]
    got = definition(x, counts)
    for m in range(3):
        for c in range(3):
            col = x[:, off[m]:off[m + 1], c]
            want = rn.everything(col, Q)
            assert abs(rn.geyer(rn.zscores(rn.pool_of(col)))[2]) > 1e-9
            for name, v in want.items():
                assert rn.close(got[name][m, c], v, 1e-10), (name, m, c, got[name][m, c], v)
    alone = definition(x[:, 4:12])   # a member is its own chain; no counts: no member axis
    for name in got:
        assert np.array_equal(alone[name], got[name][1]), name
    if n % 2:                        # an odd n' leaves the middle row out of everything
        y = x.copy()
        y[n // 2] += 1.0
        for name, v in definition(y, counts).items():
            assert np.array_equal(v, got[name]), name
    with pytest.raises(ValueError, match='too short'):
        diagnostics.rank_rhat(x[:3])
    with pytest.raises(ValueError):
        diagnostics.ess(x, 'sd')
    with pytest.raises(ValueError):
        diagnostics.mcse(x, q=[1.0])


# h = 75 and 100: the positive sequence runs over several pairs and the monotone sequence levels some of them -- the branches
# the short chains above never reach.  The bar is the one above, for the same reasons.
@pytest.mark.parametrize('n, W, rho', [(150, 4, 0.8), (151, 6, 0.9), (200, 3, 0.9)])
def test_geyers_sequences_over_many_lags_against_the_loops(n, W, rho):
    pairs = levelled = 0
    for seed in range(4):
        pool = rn.pool_of(rn.ar1(n, W, rho, seed))
        for y in (pool, rn.zscores(pool), (pool <= np.quantile(pool, 0.05)).astype(float)):
            want, max_t, end, lev = rn.geyer(y)
            assert abs(end) > 1e-9
            assert rn.close(diagnostics.ess_of(y), want, 1e-10), (seed, max_t)
            A, mv, bt = diagnostics.chain_acov(y)
            assert diagnostics.geyer_tau(A, mv, bt, y.shape[0], y.size)[1] == max_t
            short = diagnostics.geyer_tau(A[:max_t + 3], mv, bt, y.shape[0], y.size)   # a prefix that holds the end decides the same
            assert short == diagnostics.geyer_tau(A, mv, bt, y.shape[0], y.size)
            assert diagnostics.geyer_tau(A[:max(max_t, 2)], mv, bt, y.shape[0], y.size) == (None, None) or max_t < 2
            pairs, levelled = max(pairs, max_t), levelled + lev
    print('longest sequence, pairs levelled:', pairs, levelled)
    assert pairs >= 7 and levelled >= 1


def test_get_rhat_is_still_the_split_rhat_bit_for_bit():
    s = EnsembleSampler(12, 2, gauss, vectorize=True, seed=4)
    s.run_mcmc(np.random.default_rng(3).normal(size=(12, 2)), 50)
    assert np.array_equal(s.get_rhat(), diagnostics.split_rhat(s.get_chain()))
    assert np.array_equal(s.get_rhat(discard=5, thin=3, cols=[1]), diagnostics.split_rhat(s.get_chain(discard=5, thin=3)[:, :, [1]]))
    assert not np.array_equal(s.get_rhat(), s.get_rank_rhat()['rhat'])


def test_ranks_against_rankdata():
    rng = np.random.default_rng(0)
    for v in (rng.normal(size=1001), rng.integers(0, 7, 500).astype(float), np.array([0.0, -0.0, 1.0, -1.0, 0.0, 5e-324, -5e-324]),
              np.repeat(3.0, 9)):
        r = diagnostics.average_ranks(v)
        assert np.array_equal(r, scipy.stats.rankdata(v, method='average')) and np.array_equal(2 * r, np.round(2 * r))
    assert diagnostics.average_ranks([0.0, -0.0, 1.0]).tolist() == [1.5, 1.5, 3.0]


def test_ndtri_against_scipy():
    for S in (8, 750000):
        p = (np.arange(1, S + 1) - 0.375) / (S + 0.25)
        want = scipy.special.ndtri(p)
        q = np.abs(p - 0.5)
        r = np.sqrt(-np.log(np.minimum(p, 1.0 - p)))
        if S == 750000:   # the central branch, both tail branches' first, and on both sides
            assert np.any(q <= 0.425) and np.any((q > 0.425) & (p < 0.5)) and np.any((q > 0.425) & (p > 0.5)) and np.all(r[q > 0.425] <= 5.0)
        assert rn.close(diagnostics.ndtri(p), want, 1e-14)
    p = np.array([1e-300, 1e-40, 1e-12, 1e-11, 1.0 - 1e-12, 1.0 - 1e-15])   # r > 5: the far branch, both tails
    assert np.all(np.sqrt(-np.log(np.minimum(p, 1.0 - p))) > 5.0)
    assert rn.close(diagnostics.ndtri(p), scipy.special.ndtri(p), 1e-14)
    assert diagnostics.ndtri(0.5) == 0.0 and diagnostics.ndtri(0.0) == -np.inf and diagnostics.ndtri(1.0) == np.inf
    assert np.isnan(diagnostics.ndtri([-0.1, 1.1, np.nan])).all()


def test_special_values_stay_in_their_member_and_column():
    x, counts = data(10, 18, 4), [4, 8, 6]
    clean = definition(x, counts)
    x[:, 0:4, 1] = 7.0            # member 0: a constant column
    x[3, 5, 0] = np.nan           # member 1: a NaN
    x[8, 17, 2] = -np.inf         # member 2: -inf
    got = definition(x, counts)
    for name, v in got.items():
        bad = np.isnan(v).reshape(3, 3, -1).all(axis=2)
        assert bad.tolist() == [[False, True, False], [True, False, False], [False, False, True]], name
        assert np.array_equal(v[~bad], clean[name][~bad]), name
    # +0 and -0 tie: flipping the zeros' signs changes nothing
    z = np.random.default_rng(1).integers(-1, 2, (12, 4, 1)).astype(float)
    flipped = np.where(z == 0.0, -0.0, z)
    for name, v in definition(z).items():   # (an upper quantile is the largest of three values: that indicator is constant, NaN)
        assert np.array_equal(v, definition(flipped)[name], equal_nan=True) and (name.startswith('ess_') or np.all(np.isfinite(v[..., :2]))), name


def test_what_the_classic_split_rhat_misses():
    """8 walkers x 2,000 rows, seed 1.  AR(1) at rho = 0.5 with walker 0 scaled by 3: split R-hat measures 1.00007, the folded
    rank-normalised one 1.0849.  Cauchy draws with walker 0 shifted by 3: split 1.0003, rank-normalised bulk 1.0633."""
    x = rn.ar1(2000, 8, 0.5, 1)
    x[:, 0] *= 3.0
    c = np.random.default_rng(1).standard_cauchy((2000, 8))
    c[:, 0] += 3.0
    r, rc = diagnostics.rank_rhat(x[:, :, None]), diagnostics.rank_rhat(c[:, :, None])
    print(diagnostics.split_rhat(x[:, :, None]), r, diagnostics.split_rhat(c[:, :, None]), rc)
    assert diagnostics.split_rhat(x[:, :, None])[0] < 1.01 and r['folded'][0] > 1.05 and r['rhat'][0] == r['folded'][0]
    assert diagnostics.split_rhat(c[:, :, None])[0] < 1.01 and rc['bulk'][0] > 1.03


def test_ess_of_an_ar1_chain_and_of_metropolis_like_repeats():
    """AR(1), rho = 0.95, 50 x 15,000: S (1 - rho) / (1 + rho) = 19,231; measured 18,941 (bulk).  Repeats: every row is the
    row before it with probability 0.65, else a fresh normal draw (65 % of the pool tied with a neighbour) -- ranks with ties
    and the plain values must tell the same story: measured 3,545.4 (bulk) and 3,543.7 (mean)."""
    x = rn.ar1(15000, 50, 0.95, 1)[:, :, None]
    bulk = diagnostics.ess(x, 'bulk')[0]
    print('ar1 bulk', bulk)
    assert abs(bulk - 19230.77) < 0.1 * 19230.77
    rng = np.random.default_rng(3)
    n, W = 2000, 8
    fresh, keep = rng.standard_normal((n, W)), rng.random((n, W)) < 0.65
    y = fresh.copy()
    for i in range(1, n):
        y[i] = np.where(keep[i], y[i - 1], fresh[i])
    assert 0.6 < np.mean(y[1:] == y[:-1]) < 0.7
    b, m = diagnostics.ess(y[:, :, None], 'bulk')[0], diagnostics.ess(y[:, :, None], 'mean')[0]
    print('repeats bulk, mean', b, m)
    assert np.isfinite(b) and np.isfinite(m) and abs(b - m) < 0.05 * m


def gauss(x):
    return -0.5 * np.sum(x ** 2, axis=1)


def protocol(tmp, ess, nsteps=4000):
    s = EnsembleSampler(20, 2, gauss, vectorize=True, seed=5)
    d = str(tmp / 'ess_{}'.format(ess))
    os.makedirs(d)
    run_reference_protocol(s, np.random.default_rng(2).normal(size=(20, 2)), 100, nsteps, nthin=100, dirname=d, fname='run', ess=ess)
    return s, d


def test_the_protocols_ess_option(tmp_path):
    """ess=None is today's run and writes no _ess.txt.  ess=1.0 (met as soon as there is a number) stops at the same check with
    the same files and one more, whose last line is the minimum of the stored chain's bulk and tail ESS.  A bound nothing meets
    keeps the run going past that check, on the same chain."""
    plain, d0 = protocol(tmp_path, None)
    rows = len(plain._chain)
    assert rows < 3000 and not [f for f in os.listdir(d0) if 'ess' in f]
    both, d1 = protocol(tmp_path, 1.0)
    assert len(both._chain) == rows and np.array_equal(both.get_chain(), plain.get_chain())
    assert sorted(os.listdir(d1)) == sorted(os.listdir(d0) + ['run_ess.txt'])
    for f in os.listdir(d0):
        assert open(os.path.join(d0, f), 'rb').read() == open(os.path.join(d1, f), 'rb').read(), f
    lines = [float(v) for v in open(os.path.join(d1, 'run_ess.txt')).read().split()]
    want = min(np.min(both.get_ess(kind='bulk')), np.min(both.get_ess(kind='tail')))
    assert len(lines) == (rows - 1) // 100 + 1 and np.isnan(lines[0]) and lines[-1] == want and want > 1.0
    print('rows, min ESS at the stop:', rows, lines[-1])
    strict, _ = protocol(tmp_path, 1e9, nsteps=rows + 250)
    assert len(strict._chain) == rows + 250 and np.array_equal(strict.get_chain()[:rows], plain.get_chain())


def test_group_and_ladder_samplers_on_the_host(tmp_path):
    counts = [8, 12]
    g = GroupSampler(counts, 2, lambda qs: [gauss(q) for q in qs], seeds=[1, 2])
    p0s = [np.random.default_rng(k).normal(size=(n, 2)) for k, n in enumerate(counts)]
    g.run_mcmc(p0s, 60)
    single = EnsembleSampler(8, 2, gauss, vectorize=True, seed=1)
    single.run_mcmc(p0s[0], 60)
    for k in range(2):
        x = g.get_chain(k, discard=4, thin=2)
        rr = g.get_rank_rhat(discard=4, thin=2)
        assert rr['rhat'].shape == (2, 2) and sorted(rr) == ['bulk', 'folded', 'rhat']
        for name in rr:
            assert np.array_equal(rr[name][k], diagnostics.rank_rhat(x)[name]) and np.array_equal(rr[name][k], g.get_rank_rhat(k, 4, 2)[name])
        for kind in ('bulk', 'tail', 'mean'):
            assert np.array_equal(g.get_ess(discard=4, thin=2, kind=kind)[k], diagnostics.ess(x, kind))
        assert np.array_equal(g.get_mcse(k, discard=4, thin=2, cols=[1], q=[0.5])['quantiles'], diagnostics.mcse(x[:, :, [1]], [0.5])['quantiles'])
    assert np.array_equal(single.get_ess(kind='tail'), g.get_ess(0, kind='tail')) and single.get_ess().shape == (2,)
    assert np.array_equal(single.get_rank_rhat()['rhat'], np.maximum(single.get_rank_rhat()['bulk'], single.get_rank_rhat()['folded']))
    assert single.get_mcse()['quantiles'].shape == (2, 3) and single.get_mcse()['mean'].shape == (2,)
    with pytest.raises(ValueError):
        single.get_ess(kind='sd')
    with pytest.raises(ValueError, match='too short'):
        single.get_ess(discard=58)
    runs = {}
    for ess in (None, 1e9):
        s = GroupSampler(counts, 2, lambda qs: [gauss(q) for q in qs], seeds=[1, 2])
        d = tmp_path / str(ess)
        d.mkdir()
        run_group_protocol(s, p0s, 10, 60, nthin=20, dirname=str(d), ess=ess)
        runs[ess] = sorted(os.path.relpath(os.path.join(r, f), str(d)) for r, _, fs in os.walk(str(d)) for f in fs)
    assert not [f for f in runs[None] if 'ess' in f]
    assert sorted(runs[None] + ['run0/run0_ess.txt', 'run1/run1_ess.txt']) == runs[1e9]
    assert len(open(str(tmp_path / '1000000000.0' / 'run1' / 'run1_ess.txt')).read().split()) == 3

    t = TemperedSampler(8, 2, gauss, lambda q: q[:, 0] * 0, betas=[1.0, 0.5, 0.2], seed=3)
    t.run_mcmc(np.random.default_rng(5).normal(size=(3, 8, 2)), 30)
    every = t.get_ess(t=None, discard=3, kind='tail')
    assert every.shape == (3, 2) and np.array_equal(t.get_ess(discard=3, kind='tail'), every[0])
    for r in range(3):
        assert np.array_equal(every[r], diagnostics.ess(t.get_chain(t=r, discard=3), 'tail'))
        assert np.array_equal(t.get_rank_rhat(t=r)['folded'], t.get_rank_rhat(t=None)['folded'][r])
    assert t.get_mcse(t=None, cols=[1])['quantiles'].shape == (3, 1, 3) and t.get_mcse(cols=[1])['mean'].shape == (1,)
