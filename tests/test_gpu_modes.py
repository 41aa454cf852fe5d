"""GPU: the posterior's modes of a device series (include/msx.h, msx_series_modes / msx_series_mode_labels;
csrc/mode_kernels.h) against the definition (mcmc_spec_amd.modes), start by start: weights, means,
covariances and loglik to 1e-9 relative -- a mean against its own raw-unit value, a covariance element against sd_i sd_j of its
component (an off-diagonal element of a mixture component can be zero), the tolerance section 21 uses for fixed-order device
sums against their NumPy definition -- niter and status equal; the labels of every sample; the same bits whatever the
arrangement of the rows and the launch; the samples by mode; the resident samplers; every refusal.  Chains are drawn from
known mixtures (tests/modes_cases.py); selections n' of 4, 63, 64, 65, 257 and 4,099 rows (the last crosses the 4,096-row
tile), members of 2, 6 and 4 walkers."""
import ctypes as C

import numpy as np
import pytest

import common
import modes_cases as mc
from mcmc_spec_amd import modes, summary
from test_gpu_group_chain import spread
from test_gpu_group_tempered import inside, solo_of
from test_gpu_rhat import series_ctx
from test_gpu_target_group import mixed_engines

pytestmark = pytest.mark.gpu

COUNTS = [2, 6, 4]
NW = sum(COUNTS)
NROWS = 12400              # the longest selection: n' = 4,099 at discard 5, thin 3 ends at row 12,299
FLOATS = ('weight', 'mean_z', 'cov_z', 'mean', 'cov', 'loglik', 'bic')
EXACT = ('niter', 'status', 'nbad', 'count', 'best')
WORST = {'rel': 0.0}


def chain8():
    """(series, rows (NROWS, 12, 8)): three modes (0.6 / 0.3 / 0.1; the third away from the first along columns 1 and 3) in
    the fit's units, two more columns (log g of the two stars), 30 % repeated rows; no mean near zero."""
    if 'modes_series' not in common._cache:
        from mcmc_spec_amd import _lib
        rng = np.random.default_rng(23)
        x, light = mc.scaled(NROWS, NW, 7, heavy=0.7)
        third = (rng.random((NROWS, NW)) < 0.15) & ~light
        x[third] += mc.WIDTH * np.array([0.0, 6.0, 0.0, 6.0, 0.0, 0.0])
        extra = np.array([4.7, 5.0]) + np.array([0.05, 0.08]) * rng.normal(size=(NROWS, NW, 2))
        extra[:, :, 0] += 0.04 * (x[:, :, 0] - mc.CENTER[0]) / mc.WIDTH[0]
        rows = np.ascontiguousarray(np.concatenate([x, extra], axis=2))
        s = _lib.Series(series_ctx(), NW, 8, COUNTS)
        s.append(rows)
        common._cache['modes_series'] = (s, rows)
    return common._cache['modes_series']


def compare(dev, ref, tol=1e-9):
    """The device's result against the definition's, start by start."""
    for name in EXACT:
        assert np.array_equal(getattr(dev, name), getattr(ref, name)), (name, getattr(dev, name), getattr(ref, name))
    sd_z = np.sqrt(np.diagonal(ref.cov_z, axis1=-2, axis2=-1))
    sd = np.sqrt(np.diagonal(ref.cov, axis1=-2, axis2=-1))
    scales = {'weight': np.abs(ref.weight), 'loglik': np.abs(ref.loglik), 'bic': np.abs(ref.bic), 'mean': np.abs(ref.mean),
              'mean_z': sd_z, 'cov_z': sd_z[..., :, None] * sd_z[..., None, :], 'cov': sd[..., :, None] * sd[..., None, :]}
    for name in FLOATS:
        a, b = getattr(dev, name), getattr(ref, name)
        assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), name
        ok = ~np.isnan(b)
        rel = np.max(np.abs(a - b)[ok] / scales[name][ok]) if ok.any() else 0.0
        WORST['rel'] = max(WORST['rel'], float(rel))
        assert rel <= tol, (name, rel)
    print('worst relative difference so far: {:.3e}'.format(WORST['rel']))


def both(series, rows, n, discard, thin, cols, ncomp, **kw):
    dev = modes.fit_device(series, n, cols=cols, ncomp=ncomp, discard=discard, thin=thin, **kw)
    ref = modes.fit(rows[:n], list(series.counts), cols=cols, ncomp=ncomp, discard=discard, thin=thin, **kw)
    compare(dev, ref)
    return dev, ref


# (discard, thin, cols, ncomp, max_iter): the four selections, 1, 2, 6 and 8 columns, 1 to 3 components
SMALL = ((3, 2, [1], 1, 50), (0, 1, [3, 0], 2, 50))
CASES = SMALL + ((0, 7, [0, 1, 2, 3, 4, 5], 2, 50), (5, 3, None, 2, 30), (0, 1, [1, 3], 3, 50), (3, 2, [0, 1, 2, 3, 4, 5], 3, 25))
LARGE = ((0, 1, [0, 1, 2, 3, 4, 5], 2, 12), (5, 3, [3, 1], 3, 40), (3, 2, [1], 1, 50))


@pytest.mark.parametrize('np_', [4, 63, 64, 65, 257, 4099])
def test_the_fit_against_the_definition_start_by_start(np_):
    series, rows = chain8()
    for discard, thin, cols, ncomp, max_iter in (SMALL if np_ == 4 else LARGE if np_ == 4099 else CASES):
        n = discard + (np_ - 1) * thin + 1
        dev, ref = both(series, rows, n, discard, thin, cols, ncomp, max_iter=max_iter)
        d = 8 if cols is None else len(cols)
        assert dev.weight.shape == (3, d if ncomp > 1 else 1, ncomp) and list(dev.count) == [np_ * c for c in COUNTS]
        # the selection alone counts: the same n' rows from a larger n
        if thin > 1:
            again = modes.fit_device(series, n + thin - 1, cols=cols, ncomp=ncomp, discard=discard, thin=thin, max_iter=max_iter)
            assert all(np.array_equal(getattr(again, k), getattr(dev, k), equal_nan=True) for k in FLOATS + EXACT)


def test_one_gaussian_and_the_two_mode_target():
    from mcmc_spec_amd import _lib
    for x, want in ((mc.one_gauss(257, NW, 3), -1.0), (mc.two_mode(257, NW, 1), 1.0)):
        s = _lib.Series(series_ctx(), NW, 6, COUNTS)
        s.append(x)
        one, _ = both(s, x, 257, 0, 1, None, 1)
        two, ref = both(s, x, 257, 0, 1, None, 2)
        m = np.arange(3)
        assert np.all(np.sign(one.bic[m, one.best] - two.bic[m, two.best]) == want)
        s.close()


def labelled(series, rows, n, discard, thin, cols, ncomp, min_gap, **kw):
    """The definition's labels of its own best fit, after the host check that none of them is near a tie; then the device's
    under the same parameters."""
    ref = modes.fit(rows[:n], list(series.counts), cols=cols, ncomp=ncomp, discard=discard, thin=thin, **kw)
    gap = min(g.min() for g in modes.label_gaps(ref, rows[:n], list(series.counts))) if ncomp > 1 else np.inf
    print('smallest gap between the two largest lp_k:', gap)
    assert gap >= min_gap
    want, wcnt = modes.labels(ref, rows[:n], list(series.counts))
    w, mu, cv = ref.params()
    got, cnt = series.mode_labels(n, discard, thin, ref.cols, ref.center, ref.scale, w, mu, cv)
    assert got.dtype == np.uint8 and got.shape == want.shape and np.array_equal(got, want) and np.array_equal(cnt, wcnt)
    return ref, want, wcnt


@pytest.mark.parametrize('case', [(257, 0, 1, None, 2), (4099, 5, 3, [0, 1, 3], 3), (65, 0, 7, [0, 3], 2), (64, 3, 2, [1], 1)])
def test_the_labels_of_every_sample(case):
    series, rows = chain8()
    np_, discard, thin, cols, ncomp = case
    labelled(series, rows, discard + (np_ - 1) * thin + 1, discard, thin, cols, ncomp, 1e-6, max_iter=30)


def test_the_labels_of_one_gaussian_cut_in_two():
    from mcmc_spec_amd import _lib
    x = mc.one_gauss(257, NW, 3)
    s = _lib.Series(series_ctx(), NW, 6, COUNTS)
    s.append(x)
    labelled(s, x, 257, 0, 1, None, 2, 1e-6)
    dev = modes.fit_device(s, 257)
    lab, cnt = dev.labels()
    assert np.array_equal(cnt.sum(axis=1), dev.count) and lab.max() <= 1
    s.close()


def outputs(series, n, discard, thin, cols, ncomp, **kw):
    f = modes.fit_device(series, n, cols=cols, ncomp=ncomp, discard=discard, thin=thin, **kw)
    lab, cnt = f.labels()
    return [getattr(f, k) for k in FLOATS + EXACT] + [lab, cnt]


def same_bits(a, b):
    assert len(a) == len(b) and all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_the_same_bits_across_arrangements():
    from mcmc_spec_amd import _lib
    series, rows = chain8()
    cols, n, discard, thin = [0, 1, 3, 5], 9000, 5, 2        # n' = 4,498: two tiles
    want = outputs(series, n, discard, thin, cols, 2, max_iter=20)
    ctx = series_ctx()
    # appended in pieces with a growth in between, and a sentinel row past n
    for cap in (0, 5000):
        s = _lib.Series(ctx, NW, 8, COUNTS, cap_hint=cap)
        s.append(rows[:433])
        s.append(rows[433:n])
        s.append(np.full((1, NW, 8), 1e300))
        s.append(np.full((1, NW, 8), np.nan))
        same_bits(outputs(s, n, discard, thin, cols, 2, max_iter=20), want)
        s.close()
    # the pre-thinned series
    s = _lib.Series(ctx, NW, 8, COUNTS)
    s.append(rows[:n][discard::thin])
    same_bits(outputs(s, s.rows, 0, 1, cols, 2, max_iter=20), want)
    # one job per launch: every start alone, and every member alone in a series of its own
    full = modes.fit_device(series, n, cols=cols, ncomp=2, discard=discard, thin=thin, max_iter=20)
    for st in range(4):
        one = modes.fit_device(series, n, cols=cols, ncomp=2, discard=discard, thin=thin, max_iter=20, center=full.center, scale=full.scale,
                               split_col=[st], split_at=full.split_at[:, st:st + 1])
        for k in ('weight', 'mean_z', 'cov_z', 'loglik', 'niter', 'status'):
            assert np.array_equal(getattr(one, k)[:, 0], getattr(full, k)[:, st]), (k, st)
    off = np.concatenate([[0], np.cumsum(COUNTS)])
    for m in range(3):
        alone = _lib.Series(ctx, COUNTS[m], 8)
        alone.append(rows[:n, off[m]:off[m + 1]])
        one = modes.fit_device(alone, n, cols=cols, ncomp=2, discard=discard, thin=thin, max_iter=20, center=full.center[m:m + 1],
                               scale=full.scale[m:m + 1], split_col=full.split_col, split_at=full.split_at[m:m + 1])
        for k in ('weight', 'mean_z', 'cov_z', 'loglik', 'niter', 'status', 'nbad'):
            assert np.array_equal(getattr(one, k)[0], getattr(full, k)[m]), (k, m)
        alone.close()
    s.close()


def test_the_samples_by_mode():
    from mcmc_spec_amd import _lib
    series, rows = chain8()
    n, discard, thin, cols = 8300, 3, 2, [0, 1, 3]               # n' = 4,149
    ref, want, wcnt = labelled(series, rows, n, discard, thin, cols, 3, 1e-6, max_iter=30)
    dev = modes.fit_device(series, n, cols=cols, ncomp=3, discard=discard, thin=thin, max_iter=30, ctx=series_ctx())
    parts = dev.split()
    sel = rows[:n][discard::thin]
    off = np.concatenate([[0], np.cumsum(COUNTS)])
    lab, cnt = dev.labels()
    assert np.array_equal(lab, want) and np.array_equal(cnt, wcnt) and np.array_equal(cnt.sum(axis=1), dev.count - dev.nbad)
    sm = dev.summary()
    for m in range(3):
        for j in range(3):
            expect = sel[:, off[m]:off[m + 1]].transpose(1, 0, 2)[want[:, off[m]:off[m + 1]].T == j]
            part = parts[m][j]
            assert part.rows == cnt[m, j] == len(expect) and part.nw == 1 and part.ndim == 8
            assert np.array_equal(part.read()[:, 0], expect)
            q = summary.quantiles(part, part.rows, [0.16, 0.5, 0.84])
            assert np.array_equal(q[0], np.quantile(expect, [0.16, 0.5, 0.84], axis=0).T)
            assert np.array_equal(sm['quantiles'][m, j], q[0]) and sm['count'][m, j] == len(expect)
            assert np.array_equal(sm['median'][m, j], np.median(expect, axis=0)) and np.array_equal(sm['min'][m, j], expect.min(axis=0))
    # a second call into series that hold rows already: exactly the new counts; a mode nobody is in: no rows
    w, mu, cv = dev.params()
    w2 = w.copy()
    w2[:, 2] = 0.0
    flat = [p for row in parts for p in row]
    _, cnt2 = series.mode_labels(n, discard, thin, cols, dev.center, dev.scale, w2, mu, cv, dst=flat, want_labels=False)
    assert np.all(cnt2[:, 2] == 0) and np.array_equal(cnt2.sum(axis=1), dev.count) and all(parts[m][2].rows == 0 for m in range(3))
    assert all(parts[m][j].rows == cnt2[m, j] for m in range(3) for j in range(2))
    with pytest.raises(ValueError):
        summary.quantiles(parts[0][2], 1, [0.5])
    for p in flat:
        p.close()


def test_bad_samples_enter_no_sum_and_no_mode():
    from mcmc_spec_amd import _lib
    _, rows = chain8()
    x = rows[:300, :, :6].copy()
    clean = modes.fit(x, COUNTS, cols=[0, 1, 3])
    x[7, 0, 1] = np.nan
    x[9, 4, 0] = np.inf
    x[11, 5, 3] = -np.inf
    x[13, 11, 2] = np.nan          # (not a selected column)
    s = _lib.Series(series_ctx(), NW, 6, COUNTS)
    s.append(x)
    with pytest.raises(ValueError, match='scale'):
        modes.fit_device(s, 300, cols=[0, 1, 3])
    kw = dict(center=clean.center, scale=clean.scale, split_col=clean.split_col, split_at=clean.split_at)
    dev = modes.fit_device(s, 300, cols=[0, 1, 3], ctx=series_ctx(), **kw)
    ref = modes.fit(x, COUNTS, cols=[0, 1, 3], **kw)
    compare(dev, ref)
    assert list(dev.nbad) == [1, 2, 0]
    lab, cnt = dev.labels()
    want, wcnt = modes.labels(ref, x, COUNTS)
    assert np.array_equal(lab, want) and np.array_equal(cnt, wcnt) and (lab == 255).sum() == 3 and lab[7, 0] == lab[9, 4] == lab[11, 5] == 255
    parts = dev.split()
    assert [sum(p.rows for p in row) for row in parts] == list(dev.count - dev.nbad)
    for row in parts:
        for p in row:
            p.close()
    s.close()


# ---- the resident samplers: get_modes on the chain held on the device against the same chain uploaded ---------------------------
def same_fit(a, b):
    for k in FLOATS + EXACT:
        assert np.array_equal(getattr(a, k), getattr(b, k), equal_nan=True), k
    assert np.array_equal(a.labels()[0], b.labels()[0])
    sa, sb = a.summary(), b.summary()
    assert all(np.array_equal(sa[k], sb[k], equal_nan=True) for k in sa)


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
    before = dev.get_chain().copy()
    for kw in (dict(cols=[0, 1, 4]), dict(discard=5, thin=3, cols=[4, 0], ncomp=2, max_iter=10), dict(ncomp=1)):
        a, b = dev.get_modes(**kw), host.get_modes(**kw)
        same_fit(a, b)
        up = modes.uploaded(dev.get_chain(), engines[0].ctx, **kw)
        same_fit(a, up)
        compare(a, modes.fit(dev.get_chain(), **kw))
        for r in (b, up):
            r.close()
    assert np.array_equal(dev.get_chain(), before) and dev._series.rows == 40


def test_the_resident_group_sampler():
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
    for kw in (dict(cols=[0, 1, 4]), dict(k=1, discard=3, thin=2, cols=[5, 2])):
        a, b = dev.get_modes(**kw), host.get_modes(**kw)
        same_fit(a, b)
        b.close()
    every, one = dev.get_modes(cols=[0, 1, 4]), dev.get_modes(k=2, cols=[0, 1, 4])
    assert every.k == 3 and one.k == 1 and np.array_equal(every.weight[2], one.weight[0])
    compare(one, modes.fit(dev.get_chain(2), cols=[0, 1, 4]))
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
    for kw in (dict(cols=[0, 3]), dict(t=None, cols=[0, 3]), dict(t=2, discard=2, thin=2, cols=[1, 3], ncomp=1)):
        a, b = dev.get_modes(**kw), host.get_modes(**kw)
        same_fit(a, b)
        b.close()
    assert dev.get_modes(t=None, cols=[0, 3]).k == T and dev.get_modes(cols=[0, 3]).k == 1
    compare(dev.get_modes(t=1, cols=[0, 3]), modes.fit(dev.get_chain(t=1), cols=[0, 3]))


# ---- refusals --------------------------------------------------------------------------------------------------------------------
def test_every_refusal_leaves_the_series_usable():
    from mcmc_spec_amd import _lib
    series, rows = chain8()
    lib = series.lib
    before = outputs(series, 600, 1, 3, [0, 1, 3], 2, max_iter=8)
    full = modes.fit_device(series, 600, cols=[0, 1, 3], ncomp=2, discard=1, thin=3, max_iter=8)
    dp, i32p = _lib.dptr, lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    up = lambda c: None if c is None else _lib.uptr(np.asarray(c, dtype=np.uint32))
    out = [np.empty(3 * 3 * 2), np.empty(3 * 3 * 2 * 3), np.empty(3 * 3 * 2 * 9), np.empty(9), np.zeros(9, dtype=np.int32),
           np.zeros(9, dtype=np.int32), np.zeros(3, dtype=np.int64)]

    def fit(h=series.h, n=600, discard=1, thin=3, cols=(0, 1, 3), ncols=3, center=full.center, scale=full.scale, ncomp=2, nstarts=3,
            split_col=(0, 1, 2), split_at=full.split_at, max_iter=8, tol=1e-10, ridge=1e-6, skip=None):
        center, scale = _lib.as_f64(center), _lib.as_f64(scale)
        split_col, split_at = np.asarray(split_col, dtype=np.int32), _lib.as_f64(split_at)
        ptrs = [None if i == skip else (dp(o) if o.dtype == np.float64 else i32p(o) if o.dtype == np.int32 else _lib.iptr(o))
                for i, o in enumerate(out)]
        return lib.msx_series_modes(h, n, discard, thin, up(cols), ncols, dp(center), dp(scale), ncomp, nstarts, i32p(split_col),
                                    dp(split_at), max_iter, tol, ridge, *ptrs)

    assert fit() == _lib.MSX_OK and np.array_equal(out[3].reshape(3, 3), full.loglik)
    bad_scale, nan_scale, desc = full.scale.copy(), full.scale.copy(), np.zeros((3, 1, 2))
    bad_scale[1, 2], nan_scale[0, 0] = 0.0, np.nan
    desc[:, :, 0] = 1.0
    for bad in (dict(h=None), dict(thin=0), dict(discard=-1), dict(scale=bad_scale), dict(scale=nan_scale), dict(scale=-full.scale),
                dict(ridge=-1e-6), dict(max_iter=0), dict(tol=-1.0), dict(nstarts=0), dict(ncols=0)) + tuple(dict(skip=i) for i in range(7)):
        assert fit(**bad) == _lib.MSX_ERR_INVALID, bad
    for bad in (dict(n=NROWS + 1), dict(n=0), dict(n=10, discard=1), dict(n=100, discard=100), dict(cols=(0, 8, 1)), dict(cols=None),
                dict(cols=(0,) * 9, ncols=9), dict(ncomp=0), dict(ncomp=5), dict(split_col=(0, 3, 1)), dict(split_col=(0, -1, 1)),
                dict(ncomp=3, nstarts=1, split_col=(0,), split_at=desc), dict(split_at=np.full((3, 3, 1), np.nan)),
                dict(n=13, discard=1, ncomp=4, nstarts=1, split_col=(0,), split_at=np.zeros((3, 1, 3))), dict(nstarts=65)):
        assert fit(**bad) == _lib.MSX_ERR_RANGE, bad
    # N_m <= ncomp (ncols + 1): 4 rows x 2 walkers = 8 samples against 2 x 4 (the selection itself is long enough)
    assert fit(n=11, discard=1) == _lib.MSX_ERR_RANGE and fit(n=11, discard=1, ncomp=1, nstarts=1, split_col=(0,)) == _lib.MSX_OK

    w, mu, cv = full.params()
    lab, cnt = np.empty((200, NW), dtype=np.uint8), np.zeros((3, 2), dtype=np.int64)
    ctx = series_ctx()
    dst = [_lib.Series(ctx, 1, 8) for _ in range(6)]
    wide, two = _lib.Series(ctx, 1, 6), _lib.Series(ctx, 2, 8)

    def label(h=series.h, n=600, discard=1, thin=3, cols=(0, 1, 3), ncols=3, scale=full.scale, ncomp=2, weight=w, cov=cv, counts=cnt,
              dst=None):
        arr = None if dst is None else (C.c_void_p * len(dst))(*[s.h if s is not None else None for s in dst])
        return lib.msx_series_mode_labels(h, n, discard, thin, up(cols), ncols, dp(full.center), dp(_lib.as_f64(scale)), ncomp,
                                          None if weight is None else dp(_lib.as_f64(weight)), dp(mu), dp(_lib.as_f64(cov)),
                                          lab.ctypes.data_as(C.POINTER(C.c_uint8)), None if counts is None else _lib.iptr(counts), arr)

    assert label() == _lib.MSX_OK and np.array_equal(lab, before[-2]) and np.array_equal(cnt, before[-1])
    assert label(dst=dst) == _lib.MSX_OK and [s.rows for s in dst] == list(cnt.ravel())
    neg, indef = w.copy(), cv.copy()
    neg[1, 0] = -0.5
    indef[2, 1] = -np.eye(3)
    for bad in (dict(h=None), dict(thin=0), dict(discard=-1), dict(scale=bad_scale), dict(weight=None), dict(counts=None),
                dict(dst=dst[:5] + [dst[0]]), dict(dst=dst[:5] + [wide]), dict(dst=dst[:5] + [two]), dict(dst=dst[:5] + [None])):
        assert label(**bad) == _lib.MSX_ERR_INVALID, bad
    for bad in (dict(n=NROWS + 1), dict(n=10, discard=1), dict(cols=(0, 8, 1)), dict(cols=(0,) * 9, ncols=9), dict(ncomp=0), dict(ncomp=5),
                dict(weight=neg), dict(cov=indef)):
        assert label(**bad) == _lib.MSX_ERR_RANGE, bad
    with pytest.raises(ValueError):
        modes.fit_device(series, 600, cols=[0, 8])
    with pytest.raises(ValueError):
        series.mode_labels(600, 1, 3, [0, 1, 3], full.center, full.scale, neg, mu, cv)
    # everything is as it was
    assert series.rows == NROWS and [s.rows for s in dst] == list(cnt.ravel())
    same_bits(outputs(series, 600, 1, 3, [0, 1, 3], 2, max_iter=8), before)
    assert np.array_equal(series.read(0, 8), rows[:8])
    for s in dst + [wide, two]:
        s.close()
