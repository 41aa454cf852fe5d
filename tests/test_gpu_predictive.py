"""GPU: the posterior predictive check (include/msx.h, msx_predictive_batch / msx_series_predictive;
csrc/predictive_kernels.h).  (1) The reductions against NumPy's on the spectra msx_products_spectra
emits for the same samples -- min, max and quantiles bit for bit, mean and variance to 1e-9; (2) the variance on a tight
posterior, where sums of raw squares fail; (3) residuals and the likelihood's terms against the hot path, the twin and the
oracle; (4) the numbers do not depend on the scratch budget; (5) samples that cannot be evaluated are left out; (6) a device
series gives what the batch call gives; (7) the samplers' get_predictive; (8) dist_fit = False."""
import copy

import numpy as np
import pytest

import common
import predictive_numpy as twin
import products_numpy as pn
from test_gpu_products import _spectra_case, _spectra_theta, close, engine, goldens

pytestmark = pytest.mark.gpu

Q5 = (0.0, 0.16, 0.5, 0.84, 1.0)
REDUCED = ('mean', 'var', 'min', 'max', 'quantiles', 'data_norm', 'z_mean', 'z2_mean')


def recipe(n, base=None):
    """test_batch_sizes' samples: the goldens' rows tiled, no two alike."""
    base = goldens()['bin_theta'] if base is None else base
    theta = np.array(base[np.arange(n) % len(base)], dtype=float)
    theta[:, 0] += 0.37 * (np.arange(n) // len(base))
    return theta


def same(got, want, names=REDUCED):
    assert got['count'] == want['count']
    for name in names:
        assert np.array_equal(got[name], want[name], equal_nan=True), name


# ---- 1. reductions against the parent's own spectra ----------------------------------------------------------------------
@pytest.mark.parametrize('n', [1, 2, 63, 64, 65, 257])
@pytest.mark.parametrize('which', ['B', 'K', 'C'])
def test_reductions_are_numpys_on_the_emitted_spectra(which, n):
    """B: 700 px with pad pixels and unordered wavelengths, not a multiple of 256; K: a KOI target, 1,194 px; C: a triple.
    n: one and two samples, one short of, at and one past a wave, more than one 256-thread stride."""
    from mcmc_spec_amd import predictive, products
    c, eng = _spectra_case(which)
    theta = recipe(n, _spectra_theta('C') if which == 'C' else None)
    S, _, status = products.spectra(eng, theta, median_scale=True, with_status=True)
    assert np.all(status == 0)
    got = predictive.check(eng, theta, q=Q5)
    assert got['count'] == n and np.all(got['status'] == 0)
    assert got['mean'].shape == (1 + c.nspec, S.shape[2]) and got['quantiles'].shape == (5, 1 + c.nspec, S.shape[2])
    assert np.array_equal(got['min'], S.min(axis=0)) and np.array_equal(got['max'], S.max(axis=0))
    assert np.array_equal(got['quantiles'], np.quantile(S, Q5, axis=0))
    close(got['mean'], np.mean(S, axis=0), False, 'mean {} n = {}'.format(which, n))
    if n == 1:
        assert np.all(np.isnan(got['var']))
    else:
        close(got['var'], np.var(S, axis=0, ddof=1), False, 'var {} n = {}'.format(which, n))


# ---- 2. a tight posterior ---------------------------------------------------------------------------------------------
def test_variance_of_a_tight_posterior():
    """theta_i = theta_0 (1 + 1e-4 xi_i): the values spread by about 1e-4 of their mean, so a variance from sums of raw
    squares loses about eps * 1e8 = 1e-8 of it and fails the 1e-9 bar; two passes lose about n eps * 1e4 = 3e-10.
    The case is what it claims to be when var / mean^2 of row 0 is below 1e-6 on every pixel and above 1e-10 on the bulk of
    them.  Not on all: row 0 is scaled to the data's median, which pins the pixels whose flux sits at the median (measured
    here: var / mean^2 from 2.7e-15 to 3.0e-8, 112 of the 700 pixels at or below 1e-10) -- those are tighter still, harder for every formula, and the 1e-9 bar
    below holds on them too."""
    from mcmc_spec_amd import predictive, products
    _, eng = _spectra_case('B')
    xi = np.random.default_rng(20260101).uniform(-1.0, 1.0, size=(300, 6))
    theta = goldens()['bin_theta'][0][None, :] * (1.0 + 1e-4 * xi)
    S, _, status = products.spectra(eng, theta, median_scale=True, with_status=True)
    assert np.all(status == 0)
    want = twin.two_pass_var(S)
    ratio = want[0] / np.mean(S[:, 0], axis=0) ** 2
    print('var / mean^2 on row 0: {:.3e} .. {:.3e}'.format(ratio.min(), ratio.max()))
    print('pixels at or below 1e-10: {} of {}'.format(int(np.sum(ratio <= 1e-10)), ratio.size))
    assert np.all(ratio < 1e-6) and np.median(ratio) > 1e-10
    got = predictive.check(eng, theta)
    assert got['count'] == 300
    close(got['var'], want, False, 'two-pass variance, tight posterior')


# ---- 3. residuals and terms -------------------------------------------------------------------------------------------
def _samples8(which):
    theta = _spectra_theta(which, 8)[:8].copy()
    if which == 'B':   # one sample without extinction, one with a negative A_V: no reddening (mft6.py:1161)
        assert theta[2, 2] == 0.0
        theta[3, 2] = -0.3
    return theta


@pytest.mark.parametrize('which', ['B', 'A', 'K', 'C'])
def test_residuals_and_terms(which):
    from mcmc_spec_amd import predictive, products
    c, eng = _spectra_case(which)
    theta = _samples8(which)
    assert len(theta) == 8
    got = predictive.check(eng, theta)
    assert got['count'] == 8 and np.all(got['status'] == 0)
    close(got['terms'][:, 3], -2.0 * eng.loglikelihood(theta), False, 'chi_total against the hot path, case ' + which)
    S, _ = products.spectra(eng, theta, median_scale=True)
    nc, nph = len(c.fr[2]), len(c.fr[5])
    bands_ = products.evaluate(eng, theta, ['contrast:{}'.format(f) for f in range(nc)] + ['phot:{}'.format(p) for p in range(nph)])
    want = twin.check(c, theta, S, bands_[:, :nc], bands_[:, nc:])
    for j, name in enumerate(twin.TERM_NAMES):
        exact_zero = bool(np.all(want['terms'][:, j] == 0.0))   # case A has no photometry
        assert exact_zero == (name == 'chi_phot' and nph == 0)
        close(got['terms'][:, j], want['terms'][:, j], exact_zero, '{} against the twin, case {}'.format(name, which))
    close(got['data_norm'], want['data_norm'], False, 'data_norm against the twin, case ' + which)
    close(got['z2_mean'], want['z2_mean'], False, 'z2_mean against the twin, case ' + which)
    close(got['z_mean'] / np.sqrt(want['z2_mean']), want['z_mean'] / np.sqrt(want['z2_mean']), True, 'z_mean against the twin, case ' + which)
    if which not in ('A', 'B'):
        return
    # ... and the reference's own loglikelihood, on the isochrone the engine staged
    co = copy.copy(c)
    co.matrix = pn.products_matrix()
    parts = [dict() for _ in theta]
    for p, d in zip(theta, parts):
        common.oracle_loglike(co, p, parts=d)
    for j, key in enumerate(('iic', 'icontrast', 'iphot')):
        ref = np.array([d[key] for d in parts], dtype=float)
        close(got['terms'][:, j], ref, bool(np.all(ref == 0.0)), '{} against the oracle, case {}'.format(key, which))
    dn = np.mean([d['data_norm'] for d in parts], axis=0)
    z = np.array([(d['model'] - d['data_norm']) / np.asarray(c.err) for d in parts])
    z2 = np.mean(z ** 2, axis=0)
    close(got['data_norm'], dn, False, 'data_norm against the oracle, case ' + which)
    close(got['z2_mean'], z2, False, 'z2_mean against the oracle, case ' + which)
    close(got['z_mean'] / np.sqrt(z2), np.mean(z, axis=0) / np.sqrt(z2), True, 'z_mean against the oracle, case ' + which)


# ---- 4. independence of the budget ------------------------------------------------------------------------------------
def test_the_numbers_do_not_depend_on_the_scratch_budget():
    from mcmc_spec_amd import predictive
    _, eng = _spectra_case('B')
    n, npix, rows = 65, 700, 2 + 4
    theta = recipe(n)
    ref = predictive.check(eng, theta, q=Q5)
    assert ref['count'] == n
    per_pixel = 8 * rows * n
    smallest = predictive.min_scratch_bytes(eng, n)
    assert smallest == 8 * max(npix, rows * n) and smallest // per_pixel == 1            # one pixel per tile
    tile = 300                                                                           # 300 + 300 + 100: a ragged third tile
    for budget in (per_pixel * tile + 17, smallest):
        assert budget // per_pixel in (tile, 1)
        got = predictive.check(eng, theta, q=Q5, scratch_bytes=budget)
        same(got, ref)
        assert np.array_equal(got['terms'], ref['terms']) and np.array_equal(got['status'], ref['status'])
    # one byte less is refused before anything is written
    th = np.ascontiguousarray(theta)
    marks = [np.full(s, -7.0) for s in ((4, 3, npix), (5, 3, npix), (3, npix), (n, 4))]
    status, count = np.full(n, -7, dtype=np.int32), np.full(1, -7, dtype=np.int64)
    import ctypes as C
    from mcmc_spec_amd import _lib
    q = np.array(Q5)
    rc = eng.ctx.lib.msx_predictive_batch(eng.ctx.h, _lib.dptr(th), n, 6, _lib.dptr(q), 5, smallest - 1, _lib.dptr(marks[0]),
                                          _lib.dptr(marks[1]), _lib.dptr(marks[2]), _lib.dptr(marks[3]),
                                          status.ctypes.data_as(C.POINTER(C.c_int32)), _lib.iptr(count))
    assert rc == _lib.MSX_ERR_RANGE
    assert all(np.all(m == -7.0) for m in marks) and np.all(status == -7) and count[0] == -7
    with pytest.raises(ValueError):
        predictive.check(eng, theta, scratch_bytes=smallest - 1)
    with pytest.raises(ValueError):
        predictive.check(eng, theta, q=(0.5, 1.5))


# ---- 5. samples that cannot be evaluated ------------------------------------------------------------------------------
def test_samples_that_cannot_be_evaluated_are_left_out():
    from mcmc_spec_amd import _lib, predictive
    eng = engine('B')
    theta = goldens()['bin_theta'][:5].copy()
    theta[1, 0] = 6600.0
    got = predictive.check(eng, theta, q=Q5)
    assert list(got['status']) == [0, _lib.W_VALUEERROR, 0, 0, 0] and np.all(np.isnan(got['terms'][1]))
    four = predictive.check(eng, theta[[0, 2, 3, 4]], q=Q5)
    assert got['count'] == 4 and four['count'] == 4
    same(got, four)
    assert np.array_equal(got['terms'][[0, 2, 3, 4]], four['terms'])
    theta[:, 0] = 6600.0
    none = predictive.check(eng, theta, q=Q5)
    assert none['count'] == 0 and np.all(none['status'] == _lib.W_VALUEERROR) and np.all(np.isnan(none['terms']))
    for name in REDUCED:
        assert np.all(np.isnan(none[name])), name
    with pytest.raises(_lib.MsxError):
        predictive.check(engine('B', products=False), theta)


# ---- 6. a device series -----------------------------------------------------------------------------------------------
def test_a_series_gives_what_the_batch_gives():
    from mcmc_spec_amd import _lib, predictive, summary
    engs = [_spectra_case('B')[1], _spectra_case('K')[1]]
    counts, nrows = [6, 4], 40
    pool = recipe(64)
    for e in engs:
        assert np.all(predictive.check(e, pool)['status'] == 0)
    rows = pool[np.random.default_rng(8).integers(0, len(pool), size=(nrows, sum(counts)))]
    series = _lib.Series(engs[0].ctx, sum(counts), 6, counts)
    series.append(rows)
    out, tseries = predictive.check_series(series, nrows, engs, Q5, discard=5, thin=3, terms=True)
    off = np.concatenate([[0], np.cumsum(counts)])
    tall = tseries.read(0, nrows)
    assert tseries.rows == nrows and tall.shape == (nrows, sum(counts), 4)
    for m, e in enumerate(engs):
        mine = rows[:, off[m]:off[m + 1]]
        flat = mine[5::3].reshape(-1, 6)                       # (row, walker) order: get_chain(flat=True)'s
        want = predictive.check(e, flat, q=Q5)
        assert out[m]['count'] == len(flat) and out[m]['worst_status'] == 0
        same(out[m], want)
        assert np.array_equal(tall[:, off[m]:off[m + 1]].reshape(-1, 4), predictive.check(e, mine.reshape(-1, 6))['terms'])
    # without the terms series only the selection is evaluated: the same numbers
    for a, b in zip(predictive.check_series(series, nrows, engs, Q5, discard=5, thin=3), out):
        same(a, b)
    s = summary.summary_of(tseries, nrows)
    assert s['quantiles'].shape == (2, 4, 3) and np.all(np.isfinite(s['quantiles']))
    # refusals leave both series as they were
    bad = _lib.Series(engs[0].ctx, sum(counts), 3, counts)
    ctxs, npix = [e.ctx for e in engs], [int(e.tables.prob.npix) for e in engs]
    with pytest.raises(ValueError):
        series.predictive(ctxs, npix, nrows + 1, 0, 1, Q5, 0, tseries)
    with pytest.raises(ValueError):
        series.predictive(ctxs, npix, nrows, nrows, 1, Q5, 0, tseries)
    with pytest.raises(_lib.MsxError):
        series.predictive(ctxs, npix, nrows, 0, 1, Q5, 0, bad)
    assert series.rows == nrows and tseries.rows == nrows and bad.rows == 0
    assert np.array_equal(series.read(0, nrows), rows) and np.array_equal(tseries.read(0, nrows), tall)
    for x in (series, tseries, bad):
        x.close()


# ---- 7. the samplers --------------------------------------------------------------------------------------------------
NW = 12   # the fewest walkers the samplers take at ndim 6 (nwalkers >= 2 ndim)


def _start(n, seed=9):
    from mcmc_spec_amd import synth
    c = common.golden_case('B')
    return synth.draw_walkers(n, seed=seed, tmin=c.tmin, tmax=c.tmax)


def test_sampler_get_predictive_resident_and_uploaded():
    """30 iterations on case B (12 walkers: the samplers refuse fewer than 2 ndim): the resident chain and the uploaded host
    chain give the same dict bit for bit, and it is check's on get_chain(flat=True)."""
    from mcmc_spec_amd import predictive
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    eng = engine('B')
    outs = []
    for mode in ('device', 'host'):
        s = DeviceEnsembleSampler(NW, 6, eng, seed=5, chunk=7, autocorr=mode)
        s.run_mcmc(_start(NW), 30)
        outs.append(s.get_predictive(q=Q5, discard=4, thin=3))
    assert sorted(outs[0]) == sorted(outs[1])
    same(outs[0], outs[1])
    same(outs[0], predictive.check(eng, s.get_chain(discard=4, thin=3, flat=True), q=Q5))


def test_group_sampler_get_predictive():
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    engs = [engine('B'), engine('A')]
    counts = [16, 12]
    grp = TargetGroup(engs)
    dev = DeviceGroupSampler(counts, 6, grp, seeds=[40, 41], chunk=16, autocorr='device')
    p0 = [_start(counts[k], 70 + k) for k in range(2)]
    dev.run_mcmc(p0, 30)
    got = dev.get_predictive(q=Q5, discard=4, thin=3, k=1)
    both = dev.get_predictive(q=Q5, discard=4, thin=3)
    assert len(both) == 2 and both[0]['mean'].shape[1] != both[1]['mean'].shape[1]
    same(got, both[1])
    own = DeviceEnsembleSampler(counts[1], 6, engs[1], seed=41, chunk=16, autocorr='device')
    own.run_mcmc(p0[1], 30)
    assert np.array_equal(own.get_chain(), dev.get_chain(1))
    same(got, own.get_predictive(q=Q5, discard=4, thin=3))
    grp.close()


def test_tempered_sampler_get_predictive():
    from mcmc_spec_amd import predictive
    from mcmc_spec_amd.tempered import DeviceTemperedSampler
    eng = engine('B')
    s = DeviceTemperedSampler(NW, 6, eng, betas=[1.0, 0.5, 0.25], seed=17, chunk=5, autocorr='device')
    s.run_mcmc(_start(3 * NW, 5).reshape(3, NW, 6), 12)
    got = s.get_predictive(t=1, q=Q5)
    same(got, predictive.check(eng, s.get_chain(t=1, flat=True), q=Q5))
    assert len(s.get_predictive(t=None, q=Q5)) == 3


# ---- 8. dist_fit = False ----------------------------------------------------------------------------------------------
def test_terms_without_a_fitted_distance():
    from mcmc_spec_amd import predictive
    eng = engine('A', dist_fit=False)
    theta = goldens()['nod_theta'][:4]
    assert len(theta) == 4
    got = predictive.check(eng, theta)
    assert np.all(got['status'] == 0)
    close(got['terms'][:, 3], -2.0 * eng.loglikelihood(theta), False, 'chi_total, dist_fit = False')
