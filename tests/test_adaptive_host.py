"""CPU: adaptive temperature ladders on the host (mcmc_spec_amd.tempered: ladder_exp, ladder_step, TemperedSampler(adaptive=
True)): the ladder's exponential against NumPy's, the adaptive loop against a plain-Python restatement
(tests/adaptive_numpy.py), what the rule does to a lumpy ladder and what the frozen ladder then samples, the refusals and the
bookkeeping, and what an adaptive ``DeviceTemperedSampler`` asks of a context (a recording one: no library, no GPU)."""
import numpy as np
import pytest

import common  # noqa: F401
import adaptive_numpy as an
from mcmc_spec_amd import tempered
from mcmc_spec_amd.tempered import DeviceTemperedSampler, TemperedSampler, default_betas, ladder_exp, ladder_step
from test_tempered_host import BETAS3, TemperedContext, box, gauss, mix, start, tilted

LUMPY = [1.0, 0.9, 0.8, 0.1, 0.05, 0.02]


# ---- 1. the exponential ------------------------------------------------------------------------------------------------------
def test_ladder_exp_is_exp_to_a_few_ulp():
    """1e-14 relative is a cap (about 45 units of 2^-52) over the 1.6e-15 -- 7 units -- measured on 2,000,000 points of
    [-1, 1]."""
    x = np.concatenate([np.random.default_rng(19).uniform(-1.0, 1.0, 200000), [-1.0, 1.0, 0.0, 1e-300, -1e-17]])
    got, want = ladder_exp(x), np.exp(x)
    rel = np.abs(got - want) / want
    ulp = np.abs(got - want) / np.spacing(want)
    print('ladder_exp against np.exp: max relative', rel.max(), ' max ulp', ulp.max())
    assert np.all(rel <= 1e-14)
    assert ladder_exp(0.0) == 1.0 and isinstance(ladder_exp(0.0), float) and ladder_exp(np.zeros(3)).tolist() == [1.0] * 3
    assert ladder_exp(1.0) == an.exp_plain(1.0) and ladder_exp(-1.0) == an.exp_plain(-1.0)
    assert all(ladder_exp(float(v)) == an.exp_plain(v) for v in x[:2000])      # the array path and the plain restatement


# ---- 2. one step against the plain restatement (msx_ladder_step against it: tests/test_adaptive_abi.py) -----------------------
def test_ladder_step_is_the_plain_restatement_and_keeps_its_ends():
    rng = np.random.default_rng(3)
    for betas in (default_betas(8, 1e-4), LUMPY, [1.0, 0.5, 0.25], default_betas(64, 1e-4)):
        T, nw = len(betas), 50
        for counts in (np.zeros(T - 1), np.full(T - 1, nw), np.arange(T - 1) % 2 * nw, rng.integers(0, nw + 1, T - 1)):
            for k, lag, time in ((0, 8.0, 1.0), (5, 8.0, 2.0), (123456, 1e4, 100.0)):
                got, skipped = ladder_step(betas, counts, nw, k, lag, time)
                want, wskip = an.ladder_step_plain(betas, counts, nw, k, lag, time)
                assert got.tolist() == want and skipped == wskip == 0
                assert got[0] == betas[0] and got[-1] == betas[-1] and np.all(np.diff(got) < 0.0)
    # equal swap rates move nothing much; more swaps below a rung than above it pull it towards the cold end
    same, _ = ladder_step(LUMPY, [25] * 5, 50, 0, 8.0, 1.0)
    assert np.allclose(same, LUMPY, rtol=1e-14, atol=0)
    moved, _ = ladder_step([1.0, 0.5, 0.25], [50, 0], 50, 0, 8.0, 1.0)
    assert 0.25 < moved[1] < 0.5
    for T in (1, 2):
        out, skipped = ladder_step(default_betas(T, 0.1) if T > 1 else [1.0], np.zeros(T - 1), 50, 0, 8.0, 1.0)
        assert out.tolist() == ([1.0, 0.1] if T > 1 else [1.0]) and skipped == 0


def collapsing():
    """Rungs one ulp apart: the scaled gaps renormalise onto values that no longer descend strictly."""
    return np.array([1.0, np.nextafter(0.5, 1.0), 0.5, np.nextafter(0.5, 0.0), 0.25])


def test_a_step_that_would_collapse_the_ladder_is_skipped():
    b = collapsing()
    out, skipped = ladder_step(b, [50, 0, 50, 0], 50, 0, 8.0, 1.0)
    assert skipped == 1 and out.tolist() == b.tolist()
    assert an.ladder_step_plain(b, [50, 0, 50, 0], 50, 0, 8.0, 1.0) == (b.tolist(), 1)


# ---- 3. the adaptive loop ------------------------------------------------------------------------------------------------------
def test_the_adaptive_host_loop_is_the_plain_restatement_bit_for_bit():
    T, nw, ndim = 3, 12, 3
    prior = box(2.5)
    p0 = start(nw, ndim, scale=2.0)
    kw = dict(betas=BETAS3, seed=21, moves=mix())
    s = TemperedSampler(nw, ndim, tilted, prior, adaptive=True, adaptation_lag=8, adaptation_time=2, **kw)
    twin = TemperedSampler(nw, ndim, tilted, prior, **kw)                       # (its generators only)
    coords = np.repeat(p0[None], T, axis=0).copy()
    ll, lpr = tilted(coords), prior(coords)
    betas, k = BETAS3, 0
    st = p0
    for m in (5, 6):
        st = s.run_mcmc(st, m)
        rows, betas_after, nswap, nacc, k_after, skipped = an.adaptive_run(betas, coords, ll, lpr, tilted, prior, lambda: twin._draw_steps(1), m,
                                                                           k, 8.0, 2.0)
        assert k_after == k + m == s._adapted and skipped == 0 == s.ladder_skipped
        assert np.array_equal(s.get_chain(t=None), rows[0])
        assert np.array_equal(s.get_log_like(t=None), rows[1]) and np.array_equal(s.get_log_prior(t=None), rows[2])
        assert np.array_equal(s.get_betas(), rows[3]) and s.get_betas().shape == (m, T)
        assert np.array_equal(s.betas, betas_after)
        assert np.array_equal(s.swap_fraction, nswap / (m * nw)) and np.array_equal(s.acceptance_fraction, nacc / m)
        assert np.array_equal(s.get_betas()[0], betas)                         # a run starts with the ladder the last one left
        betas, k = betas_after, k_after
        s.reset()
        assert s._adapted == k and np.array_equal(s.betas, betas) and s.get_betas().shape == (0, T)
    assert k == 11
    assert betas[0] == 1.0 and betas[2] == 0.25 and betas[1] != 0.5              # the ladder moved; its ends did not


# ---- 4. what the rule does ------------------------------------------------------------------------------------------------------
def spread(s):
    return float(s.swap_fraction.max() - s.swap_fraction.min())


def test_a_lumpy_ladder_is_evened_out_and_the_frozen_ladder_samples_each_rungs_density():
    """The experiment of DESIGN.md section 19: likelihood N(0, I_6) under the box |x_i| < 20, 50 walkers, the ladder
    1, 0.9, 0.8, 0.1, 0.05, 0.02; 1,500 adaptive iterations (adaptation_lag = 1000, adaptation_time = 10), then 1,000 with the
    ladder frozen.  The frozen run's swap fractions spread (max - min over the pairs) by <= 0.15 -- three times the worst of
    seeds 0..2, 0.047 -- where the ladder left fixed spreads by >= 0.5 (0.875-0.877).  The density check runs in 3-D under the
    box |x_i| < 50 with 40 walkers and 4,000 frozen iterations after the same 1,500 adaptive ones (in 6-D under the box of
    20 the hottest rung, sigma = 7.1, is cut at 2.8 sigma, which alone takes 4 % of its variance): every rung's variance x
    beta within +-10 % and |mean| <= 0.1 sigma, the bounds of test_each_rung_samples_its_own_density."""
    p0 = 0.1 * np.random.default_rng(1).normal(size=(50, 6))
    s = TemperedSampler(50, 6, gauss, box(20.0), betas=LUMPY, seed=0, adaptive=True, adaptation_lag=1000, adaptation_time=10)
    st = s.run_mcmc(p0, 1500)
    assert s._adapted == 1500 and s.ladder_skipped == 0
    s.reset()
    st = s.run_mcmc(st, 1000, adapt=False)
    fixed = TemperedSampler(50, 6, gauss, box(20.0), betas=LUMPY, seed=0)
    fixed.run_mcmc(p0, 1000)
    print('adapted ladder', s.betas, '\nfrozen swap fractions', s.swap_fraction, 'spread', spread(s))
    print('fixed swap fractions', fixed.swap_fraction, 'spread', spread(fixed))
    assert np.all(s.get_betas() == s.betas) and s._adapted == 1500
    assert spread(s) <= 0.15
    assert spread(fixed) >= 0.5
    assert s.betas[0] == 1.0 and s.betas[-1] == 0.02 and np.all(np.diff(s.betas) < 0.0)
    # the density of every rung of a frozen, adapted ladder
    n, nw = 4000, 40
    d = TemperedSampler(nw, 3, gauss, box(50.0), betas=LUMPY, seed=3, adaptive=True, adaptation_lag=1000, adaptation_time=10)
    st = d.run_mcmc(0.1 * np.random.default_rng(1).normal(size=(nw, 3)), 1500)
    d.reset()
    d.run_mcmc(st, n, adapt=False)
    c = d.get_chain(t=None)
    for t, beta in enumerate(d.betas):
        f = c[:, t].reshape(-1, 3)
        mean, var = f.mean(axis=0) * np.sqrt(beta), f.var(axis=0) * beta
        print('rung', t, 'beta', beta, 'max |mean| / sigma', np.abs(mean).max(), 'variance x beta', var.min(), var.max())
        assert np.all(np.abs(mean) <= 0.1) and np.all(var >= 0.9) and np.all(var <= 1.1)


# ---- 5. refusals and bookkeeping ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(adaptation_lag=0.0), dict(adaptation_lag=-1.0), dict(adaptation_lag=float('nan')),
                                dict(adaptation_lag=float('inf')), dict(adaptation_time=0.5), dict(adaptation_time=float('nan')),
                                dict(adaptation_time=float('inf')), dict(adaptation_time=-3.0)])
def test_bad_lag_and_time_are_refused(kw):
    with pytest.raises(ValueError):
        TemperedSampler(12, 3, gauss, box(5.0), betas=BETAS3, adaptive=True, **kw)
    with pytest.raises(ValueError):
        DeviceTemperedSampler(16, 6, AdaptiveEngine(), betas=BETAS3, adaptive=True, **kw)
    with pytest.raises(ValueError):
        ladder_step(BETAS3, [1, 2], 12, 0, kw.get('adaptation_lag', 8.0), kw.get('adaptation_time', 2.0))
    assert ladder_step(BETAS3, [1, 2], 12, 0, 1e-300, 1.0)[1] == 0              # the bounds themselves are taken


def test_the_evidence_is_refused_over_a_moving_ladder():
    s = TemperedSampler(12, 3, gauss, box(5.0), betas=BETAS3, seed=2, adaptive=True, adaptation_lag=8, adaptation_time=2)
    st = s.run_mcmc(start(12, 3), 6)
    moved = s.betas.copy()
    assert moved[1] != 0.5
    s.run_mcmc(st, 6, adapt=False)                                               # the freeze call: nothing moves
    assert np.array_equal(s.betas, moved) and s._adapted == 6
    assert np.all(s.get_betas()[6:] == moved) and np.array_equal(s.get_betas()[0], BETAS3) and s.get_betas(discard=6, thin=2).shape == (3, 3)
    for method in ('ti', 'ss'):
        with pytest.raises(ValueError, match='ladder'):
            s.log_evidence(blocks=2, method=method)
        with pytest.raises(ValueError, match='ladder'):
            s.log_evidence(discard=5, blocks=2, method=method)                   # one adaptive row left in
        ev = s.log_evidence(discard=6, blocks=2, method=method)
        assert np.isfinite(ev.log_z) and np.array_equal(ev.mean_log_like, s.mean_log_like(discard=6))
    assert s.mean_log_like().shape == (3,) and np.all(np.isfinite(s.mean_log_like()))   # answers either way
    want = tempered.ti_log_z(moved, s.get_log_like(t=None, discard=6).mean(axis=(0, 2)))
    assert np.isclose(s.log_evidence(discard=6, blocks=2).log_z, want, rtol=1e-12)       # over the ladder the rows ran with
    # a sampler that is not adaptive: constant rows, no counters
    f = TemperedSampler(12, 3, gauss, box(5.0), betas=BETAS3, seed=2)
    f.run_mcmc(start(12, 3), 4)
    assert np.all(f.get_betas() == BETAS3) and f._adapted == 0 and f.ladder_skipped == 0 and np.isfinite(f.log_evidence(blocks=2).log_z)
    # ... and adapts when asked to, per call
    f.run_mcmc(start(12, 3), 4, adapt=True)
    assert f._adapted == 4 and f.betas[1] != 0.5


class AdaptiveContext(TemperedContext):
    """The recording context with the three methods an adaptive run may call."""

    def tempered_adapt(self, lag, time, k0):
        self.calls.append(('adapt', lag, time, k0))

    def tempered_betas(self, slot, nsteps):
        self.calls.append(('betas', slot, nsteps))
        return np.tile(self.calls[[c[0] for c in self.calls].index('begin')][1], (nsteps, 1))

    def tempered_ladder(self):
        self.calls.append(('ladder',))
        return np.array([1.0, 0.4, 0.25]), 0, 2


class AdaptiveEngine:
    def __init__(self):
        self.ctx = AdaptiveContext()


class PlainEngine:
    def __init__(self):
        self.ctx = TemperedContext()


def test_what_the_device_sampler_asks_of_a_context():
    p0 = np.random.default_rng(0).normal(size=(16, 6))
    # not adaptive, and adaptive but frozen: the context of tests/test_tempered_host.py is enough
    for kw in (dict(), dict(adaptive=True, adaptation_lag=8, adaptation_time=2)):
        eng = PlainEngine()
        s = DeviceTemperedSampler(16, 6, eng, betas=BETAS3, seed=11, chunk=4, rng='device', **kw)
        s.run_mcmc(p0, 5, **({'adapt': False} if kw else {}))
        assert {c[0] for c in eng.ctx.calls} == {'policy', 'begin', 'drawn', 'collect', 'end'}
        assert s._adapted == 0 and np.all(s.get_betas() == BETAS3) and s.get_betas().shape == (5, 3)
    # adaptive: tempered_adapt once per run, after begin and before the first enqueue, with k0 = _adapted
    eng = AdaptiveEngine()
    s = DeviceTemperedSampler(16, 6, eng, betas=BETAS3, seed=11, chunk=4, rng='device', adaptive=True, adaptation_lag=8, adaptation_time=2)
    st = s.run_mcmc(p0, 5)
    assert s._adapted == 5 and s._drawn == 5 and s.ladder_skipped == 2 and s.betas.tolist() == [1.0, 0.4, 0.25]
    s.reset()
    assert s._adapted == 5
    s.run_mcmc(st, 6)
    assert s._adapted == 11 and s.ladder_skipped == 4
    names = [c[0] for c in eng.ctx.calls]
    assert names.count('adapt') == 2 and [c for c in eng.ctx.calls if c[0] == 'adapt'] == [('adapt', 8.0, 2.0, 0), ('adapt', 8.0, 2.0, 5)]
    for run in (names[:names.index('end') + 1], names[names.index('end') + 1:]):
        assert run.index('begin') < run.index('adapt') < run.index('drawn') and run.count('adapt') == 1
        assert run.index('ladder') == len(run) - 2 and run[-1] == 'end'       # the ladder is fetched from the run, then it ends
        assert run.count('betas') == run.count('collect') == 2
    assert np.array_equal(eng.ctx.calls[names.index('end') + 1 + 1][1], [1.0, 0.4, 0.25])   # the second run begins with the moved ladder
    # a loop left early: _adapted counts the chunks QUEUED, and the ladder is still fetched
    eng2 = AdaptiveEngine()
    s2 = DeviceTemperedSampler(16, 6, eng2, betas=BETAS3, seed=11, chunk=4, rng='device', adaptive=True)
    for i, _ in enumerate(s2.sample(st, iterations=20)):
        if i == 1:
            break
    assert [c[0] for c in eng2.ctx.calls][-2:] == ['ladder', 'end'] and s2._adapted == 8 == s2._drawn and s2.betas.tolist() == [1.0, 0.4, 0.25]
    assert eng2.ctx.calls[[c[0] for c in eng2.ctx.calls].index('adapt')] == ('adapt', 10000.0, 100.0, 0)
    # host-drawn chunks: the same calls
    eng3 = AdaptiveEngine()
    s3 = DeviceTemperedSampler(16, 6, eng3, betas=BETAS3, seed=11, chunk=4, adaptive=True)
    s3.run_mcmc(p0, 6)
    n3 = [c[0] for c in eng3.ctx.calls]
    assert n3.index('begin') < n3.index('adapt') < n3.index('fed') and s3._adapted == 6 and n3.count('betas') == n3.count('collect')
