"""CPU: split R-hat and the pooled moments on the host (mcmc_spec_amd.diagnostics) against written-out
loops; members of unequal counts; special values; the device order's twin (tests/diag_numpy.py) against the same loops; the
bimodal target of tests/test_moves_host.py, where tau passes and only R-hat tells; the protocols' ``rhat=``."""
import os

import numpy as np
import pytest

import common  # noqa: F401
import diag_numpy as dn
from mcmc_spec_amd import diagnostics
from mcmc_spec_amd.group import GroupSampler, run_group_protocol
from mcmc_spec_amd.moves import DEMove, StretchMove
from mcmc_spec_amd.sampler import EnsembleSampler, run_reference_protocol
from mcmc_spec_amd.tempered import TemperedSampler
from test_moves_host import bimodal

NAMES = ('within', 'var_plus', 'between', 'rhat')


def data(n, W, seed=0):
    """(n, W, 3): three scales, means away from zero, column 2 correlated with column 1 (no covariance near zero: the
    comparisons below are relative)."""
    rng = np.random.default_rng(seed)
    a, b = rng.normal(-300.0, 40.0, (n, W)), rng.normal(5.0, 1.0, (n, W))
    return np.stack([a, b, 0.02 + 0.003 * (0.6 * (b - 5.0) + 0.8 * rng.normal(size=(n, W)))], axis=2)


# fsum against pairwise float64 sums of at most a few thousand terms: 1e-12 is three orders above either's error
@pytest.mark.parametrize('n', [4, 5, 11])
def test_the_definition_against_written_out_loops(n):
    x = data(n, 6, n)
    want = dn.loops(x, [6])
    got = diagnostics.split_parts(x)
    for name in NAMES:
        assert got[name].shape == (1, 3) and dn.close(got[name], want[name], 1e-12), name
    assert np.array_equal(diagnostics.split_rhat(x), got['rhat'][0])
    mo = diagnostics.moments(x)
    assert mo['count'] == 6 * n and dn.close(mo['mean'], want['mean'][0], 1e-12) and dn.close(mo['cov'], want['cov'][0], 1e-12)
    assert mo['cov'].shape == (3, 3) and diagnostics.moments(x[:, :, :1])['cov'].shape == (1, 1)
    # an odd n' leaves the middle row to neither half: changing it changes the moments, not R-hat
    if n % 2:
        y = x.copy()
        y[n // 2] += 1.0
        assert np.array_equal(diagnostics.split_rhat(y), diagnostics.split_rhat(x))
        assert not np.array_equal(diagnostics.moments(y)['mean'], mo['mean'])


def test_members_of_unequal_counts():
    x, counts = data(11, 18, 3), [4, 8, 6]
    want = dn.loops(x, counts)
    got = diagnostics.split_parts(x, counts)
    mo = diagnostics.moments(x, counts)
    for name in NAMES:
        assert got[name].shape == (3, 3) and dn.close(got[name], want[name], 1e-12), name
    assert dn.close(mo['mean'], want['mean'], 1e-12) and dn.close(mo['cov'], want['cov'], 1e-12)
    assert list(mo['count']) == [44, 88, 66]
    off = [0, 4, 12, 18]
    for m in range(3):   # a member is its own chain
        assert np.array_equal(diagnostics.split_rhat(x[:, off[m]:off[m + 1]]), diagnostics.split_rhat(x, counts)[m])
    with pytest.raises(ValueError):
        diagnostics.split_rhat(x, [4, 8])
    with pytest.raises(ValueError, match='too short'):
        diagnostics.split_rhat(x[:3])


def test_special_values_stay_in_their_member_and_column():
    x, counts = data(10, 18, 4), [4, 8, 6]
    clean = diagnostics.split_parts(x, counts)
    x[:, 0:4, 1] = 7.0            # member 0: a constant column
    x[3, 5, 0] = np.nan           # member 1: a NaN
    x[8, 17, 2] = -np.inf         # member 2: -inf
    for got in (diagnostics.split_parts(x, counts), None):
        if got is None:           # ... and the device's order says the same
            got = dn.twin(x, counts)
            with np.errstate(invalid='ignore', divide='ignore'):
                got['rhat'] = np.sqrt(got['var_plus'] / got['within'])
        bad = np.isnan(got['rhat'])
        assert bad.tolist() == [[False, True, False], [True, False, False], [False, False, True]]
        assert got['within'][0, 1] == 0.0 and got['between'][0, 1] == 0.0
        assert np.allclose(got['rhat'][~bad], clean['rhat'][~bad], rtol=1e-12, atol=0)
    mo = diagnostics.moments(x, counts)
    assert mo['mean'][0, 1] == 7.0 and np.isnan(mo['mean'][1, 0]) and mo['mean'][2, 2] == -np.inf
    assert np.isnan(mo['mean']).sum() == 1 and np.isnan(mo['cov'][1, 0]).all() and np.isfinite(mo['cov'][1, 1:, 1:]).all()


# the twin's sums differ from fsum by the roundoff of <= 1,100-term float64 sums; between and cov are differences of means
# good to 1e-16 relative at |mean| / spread <= 300 / 1.2: 1e-9 leaves four orders
@pytest.mark.parametrize('n', [4, 5, 257, 515])
def test_the_twin_of_the_device_order_computes_the_definition(n):
    x, counts = data(n, 18, 100 + n), [4, 8, 6]
    tw, want = dn.twin(x, counts), dn.loops(x, counts)
    for name in ('within', 'var_plus', 'between', 'mean', 'cov'):
        assert dn.close(tw[name], want[name], 1e-9), name
    assert dn.twin(x, counts, cov=False)['cov'] is None
    assert np.array_equal(tw['cov'], np.swapaxes(tw['cov'], 1, 2))


def start():
    p0 = np.random.default_rng(2).normal(size=(50, 6))
    p0[:25, 0] -= 5.0
    p0[25:, 0] += 5.0
    return p0


def mixture():
    return [(StretchMove(), 0.5), (DEMove(), 0.4), (DEMove(gamma0=1.0), 0.1)]


def test_rhat_tells_what_tau_does_not_on_the_bimodal_target():
    """50 walkers started 25 / 25, seed 5, 3,000 iterations, the second half.  Stretch only: tau (37.9; <= 84.8) times 50
    is within reach of the rows, yet no walker has changed mode (x0 < 0 fraction 0.511 for 0.8): R-hat(x0) measured 3.58,
    required >= 2.0.  The mixture: max R-hat measured 1.081, required <= 1.15."""
    s = EnsembleSampler(50, 6, bimodal, vectorize=True, seed=5)
    s.run_mcmc(start(), 3000)
    r = s.get_rhat(discard=1500)
    print('stretch', r)
    assert r.shape == (6,) and r[0] >= 2.0 and np.all(r[1:] < 1.2)
    assert np.array_equal(r, diagnostics.split_rhat(s.get_chain(discard=1500)))
    assert np.array_equal(s.get_rhat(discard=1500, thin=3, cols=[0, 2]), diagnostics.split_rhat(s.get_chain(discard=1500, thin=3)[:, :, [0, 2]]))
    mo = s.get_moments(discard=1500)
    flat = s.get_chain(discard=1500, flat=True)
    assert mo['count'] == len(flat) and np.allclose(mo['mean'], flat.mean(axis=0)) and np.allclose(mo['cov'], np.cov(flat.T))
    m = EnsembleSampler(50, 6, bimodal, vectorize=True, seed=5, moves=mixture())
    m.run_mcmc(start(), 3000)
    r = m.get_rhat(discard=1500)
    print('mixture', r)
    assert np.max(r) <= 1.15
    with pytest.raises(ValueError, match='too short'):
        m.get_rhat(discard=2997)
    with pytest.raises(ValueError, match='too short'):
        EnsembleSampler(50, 6, bimodal, vectorize=True, seed=5).get_moments()


def protocol(tmp, rhat, nsteps=20000):
    s = EnsembleSampler(50, 6, bimodal, vectorize=True, seed=5, moves=mixture())
    d = str(tmp / 'rhat_{}'.format(rhat))
    os.makedirs(d)
    run_reference_protocol(s, start(), 300, nsteps, nthin=200, dirname=d, fname='run', rhat=rhat)
    return s, d


def test_the_protocols_rhat_option(tmp_path):
    """nburn 300, nthin 200, the mixture.  rhat=None is today's run: it stops with 6,001 rows and writes no _rhat.txt.
    rhat=1.05 stops at the same check (the maximum there measures 1.022) with the same files, and one more.  rhat=1.01 runs
    past that check (measured: to 12,601 rows, where the maximum is 1.00998); the chain does not depend on nsteps, so the
    run is cut at 6,400 here, past the two checks (6,000 and 6,200) at which the tau rule alone would have stopped it."""
    plain, d0 = protocol(tmp_path, None)
    assert len(plain._chain) == 6001
    assert not [f for f in os.listdir(d0) if 'rhat' in f]
    both, d1 = protocol(tmp_path, 1.05)
    assert len(both._chain) == 6001 and np.array_equal(both.get_chain(), plain.get_chain())
    assert sorted(os.listdir(d1)) == sorted(os.listdir(d0) + ['run_rhat.txt'])
    for f in os.listdir(d0):
        assert open(os.path.join(d0, f), 'rb').read() == open(os.path.join(d1, f), 'rb').read(), f
    lines = [float(v) for v in open(os.path.join(d1, 'run_rhat.txt')).read().split()]
    assert len(lines) == 31 and np.isnan(lines[0]) and lines[-1] == np.max(both.get_rhat()) and 1.0 < lines[-1] < 1.05
    print('max R-hat at the stop:', lines[-1])
    strict, _ = protocol(tmp_path, 1.01, nsteps=6400)
    assert len(strict._chain) == 6400 and np.array_equal(strict.get_chain()[:6001], plain.get_chain())


def test_group_and_ladder_samplers_on_the_host(tmp_path):
    def gauss(x):
        return -0.5 * np.sum(x ** 2, axis=1)

    counts = [8, 12]
    g = GroupSampler(counts, 2, lambda qs: [gauss(q) for q in qs], seeds=[1, 2])
    p0s = [np.random.default_rng(k).normal(size=(n, 2)) for k, n in enumerate(counts)]
    g.run_mcmc(p0s, 40)
    every = g.get_rhat(discard=4, thin=2)
    assert every.shape == (2, 2)
    for k in range(2):
        assert np.array_equal(every[k], diagnostics.split_rhat(g.get_chain(k, discard=4, thin=2))) and np.array_equal(every[k], g.get_rhat(k, 4, 2))
        assert np.array_equal(g.get_moments(discard=4)['cov'][k], g.get_moments(k, discard=4)['cov'])
    assert list(g.get_moments()['count']) == [320, 480]
    # the group protocol: rhat=None changes nothing; a bound nothing meets keeps every target running
    runs = {}
    for rhat in (None, 1.0):
        s = GroupSampler(counts, 2, lambda qs: [gauss(q) for q in qs], seeds=[1, 2])
        d = tmp_path / str(rhat)
        d.mkdir()
        run_group_protocol(s, p0s, 10, 60, nthin=20, dirname=str(d), rhat=rhat)
        runs[rhat] = sorted(os.path.relpath(os.path.join(r, f), str(d)) for r, _, fs in os.walk(str(d)) for f in fs)
    assert not [f for f in runs[None] if 'rhat' in f]
    assert sorted(runs[None] + ['run0/run0_rhat.txt', 'run1/run1_rhat.txt']) == runs[1.0]
    assert len(open(str(tmp_path / '1.0' / 'run1' / 'run1_rhat.txt')).read().split()) == 3

    t = TemperedSampler(8, 2, gauss, lambda q: q[:, 0] * 0, betas=[1.0, 0.5, 0.2], seed=3)
    t.run_mcmc(np.random.default_rng(5).normal(size=(3, 8, 2)), 30)
    every = t.get_rhat(t=None, discard=3)
    assert every.shape == (3, 2) and np.array_equal(t.get_rhat(discard=3), every[0])
    for r in range(3):
        assert np.array_equal(every[r], diagnostics.split_rhat(t.get_chain(t=r, discard=3)))
    mo = t.get_moments(t=None, cols=[1])
    assert mo['mean'].shape == (3, 1) and mo['cov'].shape == (3, 1, 1) and sorted(mo) == ['count', 'cov', 'mean']
    assert np.array_equal(t.get_moments(t=2, cols=[1])['mean'], mo['mean'][2])
