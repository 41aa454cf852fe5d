"""GPU: split R-hat's parts and the pooled moments of a device series (include/msx.h, msx_series_moments; csrc/diag_kernels.h;
DESIGN.md section 21).  ``within, var_plus, between, mean, cov`` equal the NumPy twin of the device's order of sums
(tests/diag_numpy.py) BIT FOR BIT and the definition (mcmc_spec_amd.diagnostics) to 1e-9 relative, at selections that put
h = n' // 2 one short of, at and one past one and two of the kernels' 256-wide tiles; then column subsets, special values, the
independence of how the rows arrived, refusals, and the four resident samplers' get_rhat / get_moments against their
autocorr='host' runs."""
import numpy as np
import pytest

import common
import diag_numpy as dn
from mcmc_spec_amd import diagnostics
from test_gpu_group_chain import spread
from test_gpu_group_tempered import group_of, inside, solo_of
from test_gpu_target_group import mixed_engines

pytestmark = pytest.mark.gpu

COUNTS = [4, 8, 6]         # less than the combine kernel's threads, unequal
NROWS = 7200               # the longest selection: n' = 1027 at thin = 7 ends at row 7183
SELECTIONS = ((0, 1), (3, 2), (0, 7))
DEVICE = ('within', 'var_plus', 'between', 'mean', 'cov')


def series_ctx():
    from test_gpu_overlap import _config2
    return _config2()[0].ctx


def appended():
    """Arbitrary rows put in with msx_series_append: (series, rows (NROWS, 18, 3)).  Three scales, means away from zero and
    column 2 correlated with column 1, so that no mean or covariance lies near zero (the comparisons are relative)."""
    if 'rhat_series' not in common._cache:
        from mcmc_spec_amd import _lib
        rng = np.random.default_rng(31)
        nw = sum(COUNTS)
        a, b = rng.normal(-300.0, 40.0, (NROWS, nw)), rng.normal(5.0, 1.0, (NROWS, nw))
        rows = np.stack([a, b, 0.02 + 0.003 * (0.6 * (b - 5.0) + 0.8 * rng.normal(size=(NROWS, nw)))], axis=2)
        s = _lib.Series(series_ctx(), nw, 3, COUNTS)
        s.append(rows)
        common._cache['rhat_series'] = (s, rows)
    return common._cache['rhat_series']


def same_bits(got, want, names=DEVICE):
    for name in names:
        assert got[name].shape == want[name].shape and np.array_equal(got[name], want[name], equal_nan=True), name


def check(series, rows, n, discard, thin, cols=None, cov=True):
    """The device against the twin (bits) and the definition (1e-9 relative: between and cov are differences of means good
    to 1e-16 relative at |mean| / spread <= 300 / 1.2, over sums of <= 18,486 terms)."""
    x = rows[:n][discard::thin]
    x = x if cols is None else x[:, :, cols]
    got = series.moments(n, discard, thin, cols, cov)
    tw = dn.twin(x, series.counts, cov)
    same_bits(got, tw, DEVICE if cov else DEVICE[:4])
    want = diagnostics.split_parts(x, series.counts)
    for name in ('within', 'var_plus', 'between', 'rhat'):
        assert dn.close(got[name], want[name], 1e-9), (name, n, discard, thin)
    mo = diagnostics.moments(x, series.counts)
    assert dn.close(got['mean'], mo['mean'], 1e-9) and np.array_equal(got['count'], mo['count'])
    if cov:
        assert dn.close(got['cov'], mo['cov'], 1e-9) and np.array_equal(got['cov'], np.swapaxes(got['cov'], 1, 2))
    else:
        assert got['cov'] is None
    return got


@pytest.mark.parametrize('np_', [4, 5, 510, 511, 512, 513, 514, 1026, 1027])
def test_the_twin_bit_for_bit_and_the_definition(np_):
    series, rows = appended()
    for discard, thin in SELECTIONS:
        n = discard + (np_ - 1) * thin + 1
        got = check(series, rows, n, discard, thin)
        assert all(np.all(np.isfinite(got[name])) for name in DEVICE + ('rhat',))
    # the selection alone counts: the same n' rows from a larger n
    thin = 7
    n = (np_ - 1) * thin + 1
    assert all(np.array_equal(series.moments(n, 0, thin)[k], series.moments(n + thin - 1, 0, thin)[k]) for k in DEVICE)


def test_a_column_subset_and_no_covariance():
    series, rows = appended()
    full = check(series, rows, 700, 5, 3)
    sub = check(series, rows, 700, 5, 3, cols=[2, 0])
    assert np.array_equal(sub['within'], full['within'][:, [2, 0]]) and np.array_equal(sub['mean'], full['mean'][:, [2, 0]])
    assert np.array_equal(sub['cov'], full['cov'][:, [2, 0]][:, :, [2, 0]])
    one = check(series, rows, 700, 5, 3, cols=[1], cov=False)
    assert np.array_equal(one['rhat'], full['rhat'][:, [1]])
    none = check(series, rows, 700, 5, 3, cov=False)
    same_bits(none, full, DEVICE[:4])


def test_special_values_stay_in_their_member_and_column():
    from mcmc_spec_amd import _lib
    _, rows = appended()
    x = rows[:600].copy()
    x[:, 0:4, 1] = 7.0            # member 0: a constant column
    x[301, 5, 0] = np.nan         # member 1: a NaN
    x[8, 17, 2] = -np.inf         # member 2: -inf
    s = _lib.Series(series_ctx(), sum(COUNTS), 3, COUNTS)
    s.append(x)
    got = s.moments(600)
    same_bits(got, dn.twin(x, COUNTS))
    clean = appended()[0].moments(600)
    bad = np.isnan(got['rhat'])
    assert bad.tolist() == [[False, True, False], [True, False, False], [False, False, True]]
    assert got['within'][0, 1] == 0.0 and got['between'][0, 1] == 0.0 and got['mean'][0, 1] == 7.0     # 0 / 0
    assert np.isnan(got['mean'][1, 0]) and got['mean'][2, 2] == -np.inf and np.isnan(got['mean']).sum() == 1
    for name in ('within', 'var_plus', 'between', 'rhat', 'mean'):
        assert np.array_equal(got[name][~bad], clean[name][~bad]), name
    untouched = np.ones((3, 3, 3), dtype=bool)
    untouched[0, 1, :] = untouched[0, :, 1] = untouched[1, 0, :] = untouched[1, :, 0] = untouched[2, 2, :] = untouched[2, :, 2] = False
    assert np.array_equal(got['cov'][untouched], clean['cov'][untouched]) and np.all(np.isfinite(got['cov'][untouched]))
    assert np.all(got['cov'][0, 1] == 0.0) and np.isnan(got['cov'][1, 0]).all() and np.isnan(got['cov'][2, 2]).all()
    s.close()


def test_the_bits_do_not_depend_on_how_the_rows_arrived():
    from mcmc_spec_amd import _lib
    series, rows = appended()
    want = series.moments(1100, 2, 2)
    for cap in (0, 1100, 1000):
        s = _lib.Series(series_ctx(), sum(COUNTS), 3, COUNTS, cap_hint=cap)
        s.append(rows[:433])
        s.append(rows[433:1100])
        same_bits(s.moments(1100, 2, 2), want)
        s.close()


def test_refusals_leave_a_following_call_unchanged():
    from mcmc_spec_amd import _lib
    series, rows = appended()
    lib = series.lib
    out = [np.empty((3, 3)) for _ in range(4)] + [np.empty((3, 3, 3))]
    up = lambda c: None if c is None else _lib.uptr(np.asarray(c, dtype=np.uint32))

    def moments(h, n, discard, thin, cols, ncols, skip=None):
        ptrs = [None if i == skip else _lib.dptr(o) for i, o in enumerate(out)]
        return lib.msx_series_moments(h, n, discard, thin, up(cols), ncols, *ptrs)

    before = series.moments(1000, 1, 3)
    assert moments(series.h, 1000, 1, 3, None, 3) == _lib.MSX_OK and np.array_equal(out[3], before['mean'])
    assert moments(series.h, 1000, 1, 3, None, 3, skip=4) == _lib.MSX_OK                   # cov may be NULL
    for bad in (dict(h=None), dict(discard=-1), dict(thin=0), dict(ncols=0), dict(ncols=-2), dict(skip=0), dict(skip=1), dict(skip=2),
                dict(skip=3)):
        kw = dict(h=series.h, n=1000, discard=1, thin=3, cols=[0, 1, 2], ncols=3)
        kw.update(bad)
        assert moments(**kw) == _lib.MSX_ERR_INVALID, bad
    for bad in (dict(n=NROWS + 1), dict(n=0), dict(n=10, discard=1), dict(n=3, discard=0, thin=1), dict(n=100, discard=100),
                dict(cols=[0, 3, 1]), dict(cols=[0, 1, _lib.col_ratio(0, 1)]), dict(cols=None, ncols=2), dict(cols=[0] * 9, ncols=9)):
        kw = dict(h=series.h, n=1000, discard=1, thin=3, cols=[0, 1, 2], ncols=3)
        kw.update(bad)
        assert moments(**kw) == _lib.MSX_ERR_RANGE, bad
    assert moments(series.h, 10, 0, 3, [0, 1, 2], 3) == _lib.MSX_OK                        # n' = 4 is enough
    with pytest.raises(ValueError):
        series.moments(9, 0, 3)
    with pytest.raises(ValueError):
        series.moments(1000, cols=[3])
    assert series.rows == NROWS
    same_bits(series.moments(1000, 1, 3), before)
    assert np.array_equal(series.read(0, 8), rows[:8])


# ---- the resident samplers: get_rhat / get_moments from the device series against the same run with autocorr='host' ------------
def near(a, b):
    """1e-9 relative (the two sides sum the same chain in different orders)."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape and np.all(np.isfinite(b))
    with np.errstate(invalid='ignore', divide='ignore'):
        print('largest relative difference:', np.max(np.abs(a - b) / np.abs(b)))
    assert np.all(np.abs(a - b) <= 1e-9 * np.abs(b)), (a, b)


def same_moments(dev, host, **kw):
    near(dev.get_rhat(**kw), host.get_rhat(**kw))
    a, b = dev.get_moments(**kw), host.get_moments(**kw)
    assert sorted(a) == sorted(b) == ['count', 'cov', 'mean']
    near(a['mean'], b['mean'])
    near(a['cov'], b['cov'])
    assert np.array_equal(a['count'], b['count'])


def unchanged_by(s, calls, snapshot):
    before = snapshot()
    calls()
    after = snapshot()
    for x, y in zip(before, after):
        if isinstance(x, dict):
            assert sorted(x) == sorted(y) and all(np.array_equal(x[n], y[n]) for n in x)
        else:
            assert np.array_equal(x, y, equal_nan=True)


def test_the_resident_ensemble_sampler():
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    c, engines = mixed_engines('B')
    p0 = spread(c, 16, 61)
    run = {}
    for mode in ('device', 'host'):
        s = DeviceEnsembleSampler(16, 6, engines[0], seed=5, chunk=7, autocorr=mode)
        s.run_mcmc(p0, 40)
        run[mode] = s
    dev, host = run['device'], run['host']
    assert np.array_equal(dev.get_chain(), host.get_chain())
    unchanged_by(dev, lambda: [same_moments(dev, host, **kw) for kw in (dict(), dict(discard=5, thin=3, cols=[4, 0]))],
                 lambda: (dev.get_chain(), dev.get_autocorr_time(quiet=True), dev.get_summary()))
    assert np.array_equal(host.get_rhat(discard=4), diagnostics.split_rhat(host.get_chain(discard=4)))
    # rows queued past the ones consumed are not part of it (get_autocorr_time's rule)
    for i, st in enumerate(dev.sample(dev.get_last_sample(), iterations=20)):
        if i == 2:
            break
    assert dev._series.rows > len(dev._chain) == 43
    near(dev.get_rhat(), diagnostics.split_rhat(dev.get_chain()))
    with pytest.raises(ValueError, match='too short'):
        dev.get_rhat(discard=40)


def test_the_resident_group_sampler_with_unequal_counts():
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    c, engines = mixed_engines('B')
    counts = [12, 18, 14]
    p0s = [spread(c, n, 40 + k) for k, n in enumerate(counts)]
    grp = TargetGroup(engines[:3])
    run = {}
    for mode in ('device', 'host'):
        s = DeviceGroupSampler(counts, 6, grp, seeds=[7, 8, 9], chunk=16, autocorr=mode)
        s.run_mcmc(p0s, 36)
        run[mode] = s
    dev, host = run['device'], run['host']

    def calls():
        for kw in (dict(), dict(k=1, discard=3, thin=2), dict(k=2, cols=[5])):
            same_moments(dev, host, **kw)
    unchanged_by(dev, calls, lambda: (dev.get_chain(1), dev.get_autocorr_time(quiet=True), dev.get_summary()))
    assert dev.get_rhat().shape == (3, 6) and dev.get_moments()['cov'].shape == (3, 6, 6)
    for k in range(3):
        near(dev.get_rhat(k), diagnostics.split_rhat(dev.get_chain(k)))
    grp.close()


def test_the_resident_ladder():
    c, engines = mixed_engines('B')
    eng, nw, T = engines[0], 12, 3
    p0 = inside(eng, c, T * nw, 71).reshape(T, nw, 6)
    run = {}
    for mode in ('device', 'host'):
        s = solo_of(eng, nw, 6, [1.0, 0.5, 0.25], 11, autocorr=mode)
        s.run_mcmc(p0, 30)
        run[mode] = s
    dev, host = run['device'], run['host']
    assert np.array_equal(dev.get_chain(t=None), host.get_chain(t=None))

    def calls():
        for kw in (dict(), dict(t=None), dict(t=2, discard=2, thin=2, cols=[1, 3])):
            same_moments(dev, host, **kw)
    unchanged_by(dev, calls, lambda: (dev.get_chain(t=None), dev.get_autocorr_time(t=None, quiet=True), dev.get_summary(t=None)))
    assert dev.get_rhat(t=None).shape == (T, 6) and dev.get_rhat().shape == (6,)
    near(dev.get_rhat(t=1), diagnostics.split_rhat(dev.get_chain(t=1)))


def test_the_resident_group_ladders():
    from mcmc_spec_amd.group import TargetGroup
    c, engines = mixed_engines('B')
    members, counts, T = engines[:2], [18, 12], 2
    betas, seeds = [[1.0, 0.5], [1.0, 0.4]], [21, 22]
    p0s = [inside(e, c, T * n, 80 + k).reshape(T, n, 6) for k, (e, n) in enumerate(zip(members, counts))]
    grp = TargetGroup(members)
    run = {}
    for mode in ('device', 'host'):
        s = group_of(grp, counts, 6, betas, seeds, autocorr=mode)
        s.run_mcmc(p0s, 24)
        run[mode] = s
    for k in range(2):
        dev, host = run['device'].target(k), run['host'].target(k)
        assert np.array_equal(dev.get_chain(t=None), host.get_chain(t=None))

        def calls():
            for kw in (dict(), dict(t=None, discard=1, thin=2), dict(t=1, cols=[0, 2])):
                same_moments(dev, host, **kw)
        unchanged_by(dev, calls, lambda: (dev.get_chain(t=None), dev.get_autocorr_time(t=None, quiet=True), dev.get_summary(t=None)))
        assert dev.get_rhat(t=None).shape == (T, 6) and dev.get_moments(t=None)['mean'].shape == (T, 6)
        near(dev.get_rhat(t=1), diagnostics.split_rhat(dev.get_chain(t=1)))
    grp.close()


def test_a_series_of_derived_columns_is_a_series_like_any_other():
    """Two rungs of 16 walkers on the products fixture's engine: the derived columns' R-hat and moments from the series
    ``products.derive`` fills equal the definition on the values it holds, and the twin bit for bit."""
    from mcmc_spec_amd import products, synth
    from mcmc_spec_amd.tempered import DeviceTemperedSampler
    from test_gpu_products import PRODUCT_COLS, engine
    eng = engine('B')
    c = common.golden_case('B')
    p0 = synth.draw_walkers(32, seed=9, tmin=c.tmin, tmax=c.tmax).reshape(2, 16, 6)
    s = DeviceTemperedSampler(16, 6, eng, betas=[1.0, 0.4], seed=5, chunk=7, rng='device', autocorr='device')
    s.run_mcmc(p0, 20)
    dst = products.derive(s._series, [eng, eng], PRODUCT_COLS, 20)
    vals = dst.read(0, 20)
    assert vals.shape == (20, 32, len(PRODUCT_COLS)) and np.all(np.isfinite(vals))
    check(dst, vals, 20, 2, 3)
    dst.close()
