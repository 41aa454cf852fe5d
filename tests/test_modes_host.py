"""CPU: the definition of the posterior's modes (mcmc_spec_amd.modes) against independent facts --
samples drawn directly from known mixtures (tests/modes_cases.py), where the mixture's maximum-likelihood fit is the
labelled subsets' moments because the modes do not overlap -- and its bookkeeping: refusals, bad samples, collapse, the tie
rules, ``get_modes`` on the host samplers."""
import inspect

import numpy as np
import pytest

import common  # noqa: F401
import modes_cases as mc
from mcmc_spec_amd import diagnostics, group, modes, sampler, tempered
from mcmc_spec_amd.group import GroupSampler
from mcmc_spec_amd.sampler import EnsembleSampler
from mcmc_spec_amd.tempered import TemperedSampler
from test_moves_host import bimodal


def test_the_two_mode_target():
    """257 x 6 samples of bimodal's Gaussians: modes 10 sigma apart leave every responsibility within e^-23 of 0 or 1, so the
    weights are the counts and the labels the sign of x0, from every one of the six starts."""
    x = mc.two_mode(257, 6, 1)
    f = modes.fit(x)
    assert f.weight.shape == (1, 6, 2) and f.mean.shape == (1, 6, 2, 6) and f.cov.shape == (1, 6, 2, 6, 6)
    assert np.all(f.status == modes.CONVERGED) and np.all(f.niter < 50) and list(f.nbad) == [0] and list(f.count) == [1542]
    heavy = np.mean(x[:, :, 0] < 0.0)
    print('heavy weight', f.weight[0, :, 0], 'fraction', heavy, 'loglik', f.loglik[0])
    assert np.all(np.abs(f.weight[0, :, 0] - heavy) <= 1e-6)
    assert np.all(np.abs(f.loglik[0] - f.loglik[0, 0]) <= 1e-9 * abs(f.loglik[0, 0]))
    for s in range(6):
        lab, cnt = modes.labels(f, x, start=s)
        assert lab.dtype == np.uint8 and np.array_equal(lab, (x[:, :, 0] >= 0.0).astype(np.uint8))
        assert list(cnt[0]) == [np.sum(x[:, :, 0] < 0.0), np.sum(x[:, :, 0] >= 0.0)]
    assert min(g.min() for g in modes.label_gaps(f, x)) >= 7.0
    assert modes.compare(x)[0] > 0.0
    # the per-mode summaries are NumPy's on the labelled samples, walker-major
    parts = f.split()
    flat = x.transpose(1, 0, 2)
    assert np.array_equal(parts[0][0], flat[flat[:, :, 0] < 0.0]) and np.array_equal(parts[0][1], flat[flat[:, :, 0] >= 0.0])
    sm = f.summary()
    assert np.array_equal(sm['quantiles'][0, 1], np.quantile(parts[0][1], [0.16, 0.5, 0.84], axis=0).T)
    assert list(sm['count'][0]) == [len(parts[0][0]), len(parts[0][1])] and np.array_equal(sm['median'][0, 0], np.median(parts[0][0], axis=0))


def test_the_scaled_chain_round_trip():
    """The fit's units (Teff ~ 3850 +- 100 .. parallax ~ 2e-3 +- 2e-5), the light mode of another shape: raw-unit means
    and covariances are those of the labelled subsets (ddof = 0, plus the ridge in raw units) to 1e-6 relative."""
    y, light = mc.scaled(257, 6, 2)
    f = modes.fit(y)
    lab, cnt = modes.labels(f, y)
    assert np.array_equal(lab.astype(bool), light) and np.all(f.status == modes.CONVERGED)
    b = f.best[0]
    flat, fl = y.reshape(-1, 6), light.reshape(-1)
    for j, sel in enumerate((~fl, fl)):
        sub = flat[sel]
        mean, cov = sub.mean(axis=0), np.cov(sub.T, ddof=0) + 1e-6 * np.diag(f.scale[0] ** 2)
        sd = np.sqrt(np.diag(cov))
        assert np.all(np.abs(f.mean[0, b, j] - mean) <= 1e-6 * np.abs(mean))
        assert np.all(np.abs(f.cov[0, b, j] - cov) <= 1e-6 * np.outer(sd, sd))
        assert abs(f.weight[0, b, j] - sel.mean()) <= 1e-6
    assert np.allclose(f.mean_z[0, b] * f.scale[0] + f.center[0], f.mean[0, b], rtol=1e-15)
    mo = diagnostics.moments(y)
    assert np.allclose(f.center[0], mo['mean'], rtol=1e-14) and np.allclose(f.scale[0], np.sqrt(np.diag(mo['cov'])), rtol=1e-14)


def test_one_gaussian_prefers_one_component():
    g = mc.one_gauss(257, 6, 3)
    d = modes.compare(g)
    print('bic1 - bic2 on one Gaussian, 1,542 samples:', d)
    assert d.shape == (1,) and d[0] < 0.0
    f = modes.fit(g, ncomp=2)
    p = 2 * (1 + 6 + 21) - 1
    assert np.array_equal(f.bic, -2.0 * f.loglik + p * np.log(1542.0))


def test_a_light_mode():
    """0.95 / 0.05 at 65 x 4 (seed 11: the column-0 start has the largest likelihood): the weight is the fraction drawn, and
    that lies within three binomial sigma of 0.95 at the 0.7 x 260 independent rows."""
    x = mc.two_mode(65, 4, 11, heavy=0.95)
    f = modes.fit(x)
    w = f.weight[0, f.best[0], 0]
    print('light mode: best start', f.best, 'weight', w, 'of', f.weight[0, :, 0])
    assert f.best[0] == 0 and abs(w - np.mean(x[:, :, 0] < 0.0)) <= 1e-6
    assert abs(w - 0.95) <= 3.0 * np.sqrt(0.95 * 0.05 / (0.7 * 260))


def test_one_component_is_the_moments():
    g = mc.one_gauss(65, 4, 5)
    f = modes.fit(g, ncomp=1, cols=[0, 2, 5])
    mo = diagnostics.moments(g[:, :, [0, 2, 5]])
    N = mo['count']
    assert f.weight.shape == (1, 1, 1) and f.weight[0, 0, 0] == 1.0 and f.niter[0, 0] == 2 and f.status[0, 0] == modes.CONVERGED
    cov = mo['cov'] * (N - 1) / N + 1e-6 * np.diag(f.scale[0] ** 2)
    sd = np.sqrt(np.diag(cov))
    assert np.all(np.abs(f.mean[0, 0, 0] - mo['mean']) <= 1e-12 * np.abs(mo['mean']))
    assert np.all(np.abs(f.cov[0, 0, 0] - cov) <= 1e-12 * np.outer(sd, sd))
    lab, cnt = modes.labels(f, g)
    assert not lab.any() and list(cnt[0]) == [260]


def test_refusals():
    x = mc.two_mode(65, 4, 1)
    const = x.copy()
    const[:, :, 3] = 2.5
    with pytest.raises(ValueError, match='scale'):
        modes.fit(const)
    assert modes.fit(const, cols=[0, 1]).weight.shape == (1, 2, 2)
    for kw in ({'ncomp': 0}, {'ncomp': 5}, {'max_iter': 0}, {'ridge': -1.0}, {'thin': 0}, {'discard': -1}, {'cols': [6]}, {'cols': []},
               {'tol': float('nan')}, {'split_col': [0], 'split_at': [[[1.0]]], 'ncomp': 3}, {'split_col': [6], 'split_at': [[[0.0]]]},
               {'split_at': [[[0.0]]]}):
        with pytest.raises(ValueError):
            modes.fit(x, **kw)
    with pytest.raises(ValueError, match='descend'):
        modes.fit(x, ncomp=3, split_col=[0], split_at=[[[1.0, 0.0]]])
    with pytest.raises(ValueError, match='more than'):
        modes.fit(x[:4, :3], ncomp=2)      # 12 samples <= 2 (6 + 1)
    with pytest.raises(ValueError):
        modes.fit(x[:3])


def test_bad_samples_are_counted_and_labelled_255():
    x = mc.two_mode(129, 6, 1)
    clean = modes.fit(x, counts=[2, 4])
    y = x.copy()
    y[7, 0, 2] = np.nan
    y[9, 3, 0] = np.inf
    y[11, 5, 5] = np.nan
    with pytest.raises(ValueError, match='scale'):
        modes.fit(y, counts=[2, 4])
    kw = dict(center=clean.center, scale=clean.scale, split_col=clean.split_col, split_at=clean.split_at)
    f = modes.fit(y, counts=[2, 4], **kw)
    assert list(f.nbad) == [1, 2] and list(f.count) == [258, 516]
    lab, cnt = modes.labels(f, y, counts=[2, 4])
    want = (x[:, :, 0] >= 0.0).astype(np.uint8)
    want[7, 0] = want[9, 3] = want[11, 5] = modes.BAD
    assert np.array_equal(lab, want) and list(cnt.sum(axis=1)) == [257, 514]
    # a column that is not selected may hold anything
    f2 = modes.fit(y, counts=[2, 4], cols=[1, 3, 4])
    assert list(f2.nbad) == [0, 0]
    # the fit of the good samples is the fit of the chain without them
    keep = np.ones(129, dtype=bool)
    keep[[7]] = False
    a = modes.fit(y[:, :1], center=clean.center[:1], scale=clean.scale[:1], split_col=clean.split_col, split_at=clean.split_at[:1])
    b = modes.fit(x[keep][:, :1], center=clean.center[:1], scale=clean.scale[:1], split_col=clean.split_col, split_at=clean.split_at[:1])
    assert np.array_equal(a.weight, b.weight) and np.array_equal(a.loglik, b.loglik) and np.array_equal(a.cov, b.cov)


def test_a_collapse_is_flagged():
    x = mc.two_mode(65, 4, 1)
    top = np.sort(x[:, :, 0].ravel())
    # a threshold above every sample: the hard assignment leaves component 1 empty -- no parameters, no iteration
    f = modes.fit(x, cols=[0], split_col=[0], split_at=[[[top[-1] + 1.0]]])
    assert f.status[0, 0] == modes.COLLAPSED and f.niter[0, 0] == 0 and np.isnan(f.loglik[0, 0]) and np.all(np.isnan(f.weight))
    assert modes.STATUS[f.status[0, 0]] == 'collapsed'
    # one sample alone in component 1: its variance is the ridge, its responsibility for itself falls just short of 1
    f = modes.fit(x, cols=[0], split_col=[0, 0], split_at=[[[(top[-1] + top[-2]) / 2.0], [0.0]]])
    assert f.status[0, 0] == modes.COLLAPSED and f.niter[0, 0] == 1 and np.isfinite(f.loglik[0, 0])
    assert f.weight[0, 0, 1] == 1.0 / 260 and f.status[0, 1] == modes.CONVERGED and f.best[0] == 1


def test_component_order_and_best_follow_the_tie_rules():
    assert list(modes._ordered(np.array([0.5, 0.5]), np.array([[1.0], [-1.0]]))) == [1, 0]
    assert list(modes._ordered(np.array([0.2, 0.5, 0.3]), np.zeros((3, 1)))) == [1, 2, 0]
    assert list(modes._ordered(np.array([np.nan, 0.5]), np.zeros((2, 1)))) == [1, 0]
    assert modes._best(np.array([-3.0, -1.0, -1.0])) == 1 and modes._best(np.array([np.nan, -5.0])) == 1
    x = mc.two_mode(65, 4, 1)
    f = modes.fit(x, split_col=[2, 0, 0], split_at=[[[0.0], [0.0], [0.0]]])
    assert f.loglik[0, 1] == f.loglik[0, 2] and f.best[0] in (0, 1) and (f.best[0] == 1 or f.loglik[0, 0] >= f.loglik[0, 1])
    assert np.all(f.weight[..., 0] >= f.weight[..., 1])
    # two equal halves, mirrored: the component with the smaller first-column mean comes first
    s = np.concatenate([x[:32], -x[:32]])
    f = modes.fit(s, cols=[0], split_col=[0], split_at=[[[0.0]]])
    assert f.weight[0, 0, 0] == f.weight[0, 0, 1] == 0.5 and f.mean[0, 0, 0, 0] < f.mean[0, 0, 1, 0]


def test_every_sampler_has_get_modes_and_the_host_ones_match_the_definition():
    sig = lambda fn: list(inspect.signature(fn).parameters)
    for cls, lead in ((sampler.EnsembleSampler, []), (sampler.DeviceEnsembleSampler, []), (group.GroupSampler, ['k']),
                      (group.DeviceGroupSampler, ['k']), (tempered.TemperedSampler, ['t']), (tempered.DeviceTemperedSampler, ['t']),
                      (tempered._TargetLadder, ['t'])):
        assert hasattr(cls, 'get_moments') and sig(cls.get_modes) == ['self'] + lead + ['ncomp', 'discard', 'thin', 'cols', 'fit_kw'], cls
        p = inspect.signature(cls.get_modes).parameters
        assert (p['ncomp'].default, p['discard'].default, p['thin'].default, p['cols'].default) == (2, 0, 1, None)

    def same(a, b):
        # (a member cut out of a wider array is summed by NumPy in another order than the same member alone: 1e-12)
        return (all(np.array_equal(getattr(a, n), getattr(b, n)) for n in ('niter', 'status', 'best', 'nbad', 'count'))
                and all(np.allclose(getattr(a, n), getattr(b, n), rtol=1e-12, atol=1e-12) for n in ('weight', 'mean_z', 'cov_z', 'loglik', 'bic')))

    p0 = np.random.default_rng(2).normal(size=(12, 6))
    p0[:9, 0] -= 5.0
    p0[9:, 0] += 5.0
    s = EnsembleSampler(12, 6, bimodal, vectorize=True, seed=5)
    s.run_mcmc(p0, 60)
    got = s.get_modes(discard=10, thin=2, cols=[0, 1, 2])
    assert same(got, modes.fit(s.get_chain(discard=10, thin=2), cols=[0, 1, 2]))
    assert abs(got.weight[0, got.best[0], 0] - 0.75) <= 1e-6      # (the stretch move alone: no walker changes mode)
    assert np.array_equal(got.labels()[0], (s.get_chain(discard=10, thin=2)[:, :, 0] >= 0).astype(np.uint8))

    g = GroupSampler([12, 12], 6, lambda qs: [bimodal(q) for q in qs], seeds=[1, 2])
    g.run_mcmc([p0, p0[::-1]], 40)
    every = g.get_modes(discard=4)
    assert every.k == 2
    for k in range(2):
        assert same(g.get_modes(k, discard=4), modes.fit(g.get_chain(k, discard=4)))
        assert np.array_equal(every.weight[k], g.get_modes(k, discard=4).weight[0])

    t = TemperedSampler(12, 6, bimodal, lambda q: q[:, 0] * 0, betas=[1.0, 0.5], seed=3)
    t.run_mcmc(np.stack([p0, p0]), 40)
    assert same(t.get_modes(discard=4, max_iter=20), modes.fit(t.get_chain(t=0, discard=4), max_iter=20))
    assert t.get_modes(t=None, discard=4).k == 2 and same(t.get_modes(t=1, discard=4), modes.fit(t.get_chain(t=1, discard=4)))
