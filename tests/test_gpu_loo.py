"""GPU: pointwise model checks (include/msx.h, msx_predictive_pointwise / msx_series_pointwise; csrc/pointwise_kernels.h;
DESIGN.md section 25).  (1) The pointwise matrix: its pixel rows average to the predictive check's z2_mean times the
likelihood's coefficient, each sample's column adds up to the hot path's log-likelihood, and the six per-observation outputs
are the definition's (mcmc_spec_amd/psis.py, pointwise_stats) on that matrix to 1e-9; (2) the bits do not depend on the
scratch budget; (3) samples that cannot be evaluated are left out; (4) a device series gives the batch call's bits; (5) the
samplers' get_loo; (6) a problem without a spectrum; (7) compare; (8) refusals."""
import numpy as np
import pytest

import common
from mcmc_spec_amd import psis
from test_gpu_predictive import NW, _start, recipe
from test_gpu_products import _spectra_case, _spectra_theta, engine, goldens

pytestmark = pytest.mark.gpu

TOL = 1e-9
KEYS = ('lppd', 'p_waic', 'elpd_waic', 'elpd_loo', 'p_loo', 'khat')


def same(got, want):
    assert got['count'] == want['count'] and got['tail_len'] == want['tail_len'] and got['n_obs'] == want['n_obs']
    for name in KEYS:
        assert np.array_equal(got[name], want[name], equal_nan=True), name
    assert got['total'] == want['total'] and got['n_bad_k'] == want['n_bad_k']


def samples(which, n):
    return recipe(n, _spectra_theta('C') if which == 'C' else None)


def case(which, n):
    """(engine, theta, loo's dict with the matrix), evaluated once per (case, n)."""
    key = ('loo_case', which, n)
    if key not in common._cache:
        _, eng = _spectra_case(which)
        theta = samples(which, n)
        common._cache[key] = (eng, theta, psis.loo(eng, theta, pointwise=True))
    return common._cache[key]


# ---- 1. the matrix and the six outputs ------------------------------------------------------------------------------------
@pytest.mark.parametrize('n', [24, 300])
@pytest.mark.parametrize('which', ['B', 'C', 'K'])
def test_the_matrix_and_the_outputs_are_the_definitions(which, n):
    """B: 700 px with pad pixels and unordered wavelengths; C: a triple; K: a KOI target, 1,194 px.  24 samples: a tail of 5,
    one lane-stride; 300: a tail of 52, more than one stride."""
    from mcmc_spec_amd import predictive
    eng, theta, got = case(which, n)
    npix, nc, nph = eng.ctx.pointwise_nobs()
    assert got['count'] == n and np.all(got['status'] == 0) and got['n_obs'] == npix + nc + nph and nc + nph > 0
    assert got['tail_len'] == min(psis.tail_len(n), n - 1)
    ll = got['pointwise']
    assert ll.shape == (npix + nc + nph, n) and np.all(np.isfinite(ll)) and np.all(ll <= 0.0)
    # the pixel rows average to coef * z2_mean of the predictive check
    chk = predictive.check(eng, theta)
    coef = (-0.5 * (nc + nph)) / npix
    d = np.abs(np.mean(ll[:npix], axis=1) / (coef * chk['z2_mean']) - 1.0)
    print('loo-figures {} n = {}: pixel rows against coef * z2_mean, worst relative {:.3e}'.format(which, n, d.max()))
    assert np.all(d <= 1e-12)
    # the filters' rows: -0.5 of the predictive check's chi_contrast and chi_phot, summed
    assert np.allclose(np.sum(ll[npix:npix + nc], axis=0), -0.5 * chk['terms'][:, 1], rtol=1e-12, atol=0.0) or nc == 0
    assert np.allclose(np.sum(ll[npix + nc:], axis=0), -0.5 * chk['terms'][:, 2], rtol=1e-12, atol=0.0) or nph == 0
    # each sample's column adds up to the hot path's log-likelihood
    want_ll = eng.loglikelihood(theta)
    d = np.abs(np.sum(ll, axis=0) / want_ll - 1.0)
    print('loo-figures {} n = {}: column sums against loglikelihood, worst relative {:.3e}'.format(which, n, d.max()))
    assert np.all(d <= TOL)
    # the six outputs are the definition's on the downloaded matrix
    want = psis.pointwise_stats(ll)
    for name in KEYS:
        inf = np.isinf(want[name])
        assert np.array_equal(np.isinf(got[name]), inf) and np.array_equal(np.isnan(got[name]), np.isnan(want[name])), name
        ok = np.isfinite(want[name])
        d = np.abs(got[name][ok] - want[name][ok]) / np.maximum(1.0, np.abs(want[name][ok]))
        print('loo-figures {} n = {}: {} against the definition, worst {:.3e}'.format(which, n, name, d.max() if d.size else 0.0))
        assert np.all(d <= TOL), name
    assert np.all(got['p_waic'] >= 0.0) and got['n_bad_k'] == int(np.sum(got['khat'] > 0.7))
    for name in KEYS[:5]:
        assert got['total'][name] == float(np.sum(got[name]))
        assert abs(got['total'][name] - want['total'][name]) <= TOL * abs(want['total'][name])
    # the split and the worst observations
    assert np.array_equal(got['pixels']['khat'], got['khat'][:npix]) and got['contrast']['lppd'].shape == (nc,) and got['phot']['lppd'].shape == (nph,)
    assert len(got['worst']) == 10 and got['worst'][0]['khat'] == np.max(got['khat']) and got['worst'][0]['wavelength'] is None


# ---- 2. independence of the budget ------------------------------------------------------------------------------------
def test_the_bits_do_not_depend_on_the_scratch_budget():
    eng, theta, ref = case('B', 300)
    npix, n = 700, 300
    smallest = 8 * max(npix, n)
    for budget in (smallest, 8 * n * 300 + 17):                 # one observation per tile; 300 + 300 + 100 pixels, then the filters
        out, status, count, tail, mat = eng.ctx.predictive_pointwise(theta, 1.0, budget, True)
        assert count == n and tail == ref['tail_len'] and np.array_equal(mat, ref['pointwise'])
        for i, name in enumerate(KEYS):
            assert np.array_equal(out[i], ref[name], equal_nan=True), name
    with pytest.raises(ValueError):
        eng.ctx.predictive_pointwise(theta, 1.0, smallest - 1)


# ---- 3. samples that cannot be evaluated ------------------------------------------------------------------------------
def test_samples_that_cannot_be_evaluated_are_left_out():
    from mcmc_spec_amd import _lib
    eng = engine('B')
    theta = recipe(30)
    theta[[1, 17], 0] = 6600.0
    got = psis.loo(eng, theta, pointwise=True)
    keep = np.delete(np.arange(30), [1, 17])
    assert got['count'] == 28 and list(np.nonzero(got['status'])[0]) == [1, 17] and got['status'][1] == _lib.W_VALUEERROR
    assert got['pointwise'].shape[1] == 28 and got['tail_len'] == min(psis.tail_len(28), 27)
    want = psis.loo(eng, theta[keep], pointwise=True)
    same(got, want)
    assert np.array_equal(got['pointwise'], want['pointwise'])
    theta[1:, 0] = 6600.0                                        # one sample left: nothing to leave out
    none = psis.loo(eng, theta)
    assert none['count'] == 1 and all(np.all(np.isnan(none[name])) for name in KEYS)


# ---- 4. a device series -----------------------------------------------------------------------------------------------
def test_a_series_gives_the_batch_calls_bits():
    from mcmc_spec_amd import _lib
    engs = [_spectra_case('B')[1], _spectra_case('K')[1]]
    counts, nrows = [6, 4], 40
    pool = recipe(64)
    rows = pool[np.random.default_rng(8).integers(0, len(pool), size=(nrows, sum(counts)))]
    series = _lib.Series(engs[0].ctx, sum(counts), 6, counts)
    series.append(rows)
    out = psis.loo_series(series, nrows, engs, discard=5, thin=3, pointwise=True)
    off = np.concatenate([[0], np.cumsum(counts)])
    for m, e in enumerate(engs):
        flat = rows[5::3, off[m]:off[m + 1]].reshape(-1, 6)        # (row, walker) order: get_chain(flat=True)'s
        want = psis.loo(e, flat, pointwise=True)
        assert out[m]['count'] == len(flat) and out[m]['worst_status'] == 0
        same(out[m], want)
        assert np.array_equal(out[m]['pointwise'], want['pointwise'])
    with pytest.raises(ValueError):
        psis.loo_series(series, nrows + 1, engs)
    with pytest.raises(ValueError):
        psis.loo_series(series, nrows, engs, discard=nrows)
    with pytest.raises(_lib.MsxError):
        psis.loo_series(series, nrows, engs, thin=0)
    assert series.rows == nrows and np.array_equal(series.read(0, nrows), rows)
    series.close()


# ---- 5. the samplers --------------------------------------------------------------------------------------------------
def test_sampler_get_loo_resident_and_uploaded():
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    eng = engine('B')
    outs = []
    for mode in ('device', 'host'):
        s = DeviceEnsembleSampler(NW, 6, eng, seed=5, chunk=7, autocorr=mode)
        s.run_mcmc(_start(NW), 30)
        outs.append(s.get_loo(discard=4, thin=3))
    same(outs[0], outs[1])
    same(outs[0], psis.loo(eng, s.get_chain(discard=4, thin=3, flat=True)))
    assert outs[0]['count'] == 9 * NW


def test_group_and_tempered_get_loo():
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    from mcmc_spec_amd.tempered import DeviceTemperedSampler
    engs = [engine('B'), engine('A')]
    counts = [16, 12]
    grp = TargetGroup(engs)
    dev = DeviceGroupSampler(counts, 6, grp, seeds=[40, 41], chunk=16, autocorr='device')
    dev.run_mcmc([_start(counts[k], 70 + k) for k in range(2)], 30)
    both = dev.get_loo(discard=4, thin=3)
    assert len(both) == 2 and both[0]['n_obs'] != both[1]['n_obs']
    for k in range(2):
        same(both[k], psis.loo(engs[k], dev.get_chain(k, discard=4, thin=3, flat=True)))
    same(dev.get_loo(discard=4, thin=3, k=1), both[1])
    grp.close()
    s = DeviceTemperedSampler(NW, 6, engs[0], betas=[1.0, 0.5, 0.25], seed=17, chunk=5, autocorr='device')
    s.run_mcmc(_start(3 * NW, 5).reshape(3, NW, 6), 12)
    same(s.get_loo(), psis.loo(engs[0], s.get_chain(t=0, flat=True)))       # rung 0: the posterior
    assert len(s.get_loo(t=None)) == 3


# ---- 6. a problem without a spectrum ----------------------------------------------------------------------------------
def test_a_problem_without_a_spectrum_has_the_filters_alone():
    import products_numpy as pn
    from mcmc_spec_amd import bands
    from mcmc_spec_amd.engine import Engine
    from test_gpu_products import golden_case, stage_products
    c = golden_case('B')
    eng = Engine(0)
    eng.stage_specs(c.specs)
    eng.stage_problem(c.data, c.err, c.fr, c.r, c.ctm, c.ptm, c.tmi, c.tma, pn.products_matrix(), nspec=c.nspec,
                      bands=bands.make_bands(c.tables, *c.vega), av_table=common.av_table_exact(), tmin=c.tmin, tmax=c.tmax,
                      prior=0, dist_fit=True, rad_prior=True, spectrum=False)
    stage_products(eng, goldens())
    theta = recipe(24)
    got = psis.loo(eng, theta, pointwise=True)
    npix, nc, nph = eng.ctx.pointwise_nobs()
    assert npix == 0 and got['n_obs'] == nc + nph == len(c.fr[2]) + len(c.fr[5]) and got['pointwise'].shape == (nc + nph, 24)
    assert np.all(np.abs(np.sum(got['pointwise'], axis=0) / eng.loglikelihood(theta) - 1.0) <= TOL)
    # the filters' terms do not depend on the spectrum term: the full problem's last rows
    assert np.array_equal(got['pointwise'], case('B', 24)[2]['pointwise'][-(nc + nph):])


# ---- 7. compare -------------------------------------------------------------------------------------------------------
def test_compare_of_two_chains_is_the_definitions():
    eng, theta, a = case('B', 300)
    shifted = theta.copy()
    shifted[:, 0] += 25.0
    b = psis.loo(eng, shifted, pointwise=True)
    got, back = psis.compare(a, b), psis.compare(b, a)
    want = psis.compare(psis.pointwise_stats(a['pointwise']), psis.pointwise_stats(b['pointwise']))
    for name in ('elpd_loo', 'elpd_waic'):
        assert got[name][0] == -back[name][0] and got[name][1] == back[name][1] and got[name][1] > 0.0
        assert abs(got[name][0] - want[name][0]) <= TOL * max(1.0, abs(want[name][0]))
        assert abs(got[name][1] - want[name][1]) <= TOL * want[name][1]
    with pytest.raises(ValueError):
        psis.compare(a, case('K', 24)[2])


# ---- 8. refusals ------------------------------------------------------------------------------------------------------
def test_refusals():
    from mcmc_spec_amd import _lib
    eng = engine('B')
    theta = recipe(24)
    with pytest.raises(_lib.MsxError):
        psis.loo(engine('B', products=False), theta)
    with pytest.raises(_lib.MsxError):
        psis.loo(eng, theta, reff=0.0)
    with pytest.raises(_lib.MsxError):
        psis.loo(eng, theta[:, :5])
    with pytest.raises(ValueError):                               # over 700 observations x 200,000 samples: past MSX_POINTWISE_MATRIX_MAX
        psis.loo(eng, np.zeros((200000, 6)), pointwise=True)
    assert 8 * sum(eng.ctx.pointwise_nobs()) * 200000 > _lib.POINTWISE_MATRIX_MAX
