"""GPU: importance reweighting of a device series (include/msx.h, msx_series_logprob / _lincomb / _weights / _wmoments /
_resample; csrc/reweight_kernels.h) against its NumPy definition, mcmc_spec_amd/reweight.py.
(1) re-scored rows carry the evaluation's bits, -inf for a rejected sample and NaN plus the status for one in error;
(2) lincomb, the weights' statistics and the weighted moments equal the definition bit for bit, the weights themselves to
the measured distance between the device library's exp and NumPy's; (3) systematic resampling draws the definition's
indices at every tile boundary and past one million samples; (4) the samplers' get_reweighted."""
import ctypes as C

import numpy as np
import pytest

import common
from mcmc_spec_amd import reweight as rw
from test_gpu_group_chain import spread
from test_gpu_group_tempered import inside, solo_of
from test_gpu_rhat import series_ctx
from test_gpu_target_group import _stage, mixed_engines

pytestmark = pytest.mark.gpu

T = rw.TILE
COUNTS = (2, 3)
NW = sum(COUNTS)
# The largest distance, in units of the last place, between the device's w = exp(logw - M) and np.exp(logw - M) over this
# file's inputs, measured on the MI355X (ROCm's exp against glibc's): DESIGN.md section 24 records it.  The tests allow one
# ulp more, so that a library update that stays within one more ulp still passes.
MEASURED_EXP_ULP = 1


def ulps(a, b):
    """The distance between two arrays of non-negative finite doubles in units of the last place."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return np.abs(a.view(np.int64) - b.view(np.int64))


def new_series(ndim, rows=None, counts=COUNTS, pieces=1, cap_hint=0):
    from mcmc_spec_amd import _lib
    s = _lib.Series(series_ctx(), sum(counts), ndim, list(counts), cap_hint=cap_hint)
    if rows is not None:
        for part in np.array_split(np.asarray(rows, dtype=np.float64).reshape(len(rows), sum(counts), ndim), pieces):
            s.append(part)
    return s


# ---- 1. msx_series_logprob -------------------------------------------------------------------------------------------------
def logprob_case():
    """Golden case B and its cropped copy as two members of 2 and 3 walkers, 7 rows; one theta outside the prior box, one
    secondary outside the isochrone table, one primary past the last grid node."""
    if 'reweight_lp' not in common._cache:
        c, engines = mixed_engines('B')
        theta = spread(c, 7 * NW, 17, 0.3).reshape(7, NW, 6)
        theta[2, 1, 3] = -0.5      # R1 < 0: outside the prior box
        theta[4, 3, 1] = 2800.0    # outside the isochrone: ValueError (likelihood), reject (posterior)
        theta[5, 0, 0], theta[5, 0, 1] = 4325.0, 3500.0   # beyond the last node: IndexError
        common._cache['reweight_lp'] = (c, engines[:2], theta, new_series(6, theta, pieces=2))
    return common._cache['reweight_lp']


def expected_logprob(engines, theta, mode):
    want, status = np.empty(theta.shape[:2]), np.empty(theta.shape[:2], dtype=np.int32)
    off = np.concatenate([[0], np.cumsum(COUNTS)])
    for m, eng in enumerate(engines):
        th = theta[:, off[m]:off[m + 1]].reshape(-1, 6)
        lp, st = eng.ctx.logprob_batch(th, mode)
        want[:, off[m]:off[m + 1]] = np.where(st == 1, -np.inf, np.where(st > 1, np.nan, lp)).reshape(-1, COUNTS[m])
        status[:, off[m]:off[m + 1]] = st.reshape(-1, COUNTS[m])
    return want, status


@pytest.mark.parametrize('mode', ['logposterior', 'logprior', 'loglikelihood'])
def test_rescored_rows_carry_the_evaluations_bits(mode):
    from mcmc_spec_amd import _lib
    c, engines, theta, series = logprob_case()
    code = rw.MODES[mode]
    want, status = expected_logprob(engines, theta, code)
    off = np.concatenate([[0], np.cumsum(COUNTS)])
    dst = rw.rescore(series, 7, engines, mode)
    got = dst.read()[:, :, 0]
    assert np.array_equal(got, want, equal_nan=True)
    assert list(dst.worst_status) == [max(0, status[:, off[m]:off[m + 1]].max()) if status[:, off[m]:off[m + 1]].max() > 1 else 0
                                      for m in range(2)]
    # the engines' own numbers, sample by sample, where the engine returns one
    for m, eng in enumerate(engines):
        fn = {'logposterior': eng.logposterior, 'logprior': eng.logprior, 'loglikelihood': eng.loglikelihood}[mode]
        ok = status[:, off[m]:off[m + 1]] <= 1
        assert np.array_equal(got[:, off[m]:off[m + 1]][ok], fn(theta[:, off[m]:off[m + 1]][ok]))
    assert got[2, 1] == -np.inf or mode == 'loglikelihood'          # outside the prior box
    if mode != 'logprior':
        assert np.all(got[status == 1] == -np.inf) and np.all(np.isnan(got[status > 1]))
    if mode == 'logposterior':
        assert (status == 1).sum() >= 2
    if mode == 'loglikelihood':
        assert np.isnan(got[4, 3]) and status[4, 3] == _lib.W_VALUEERROR and dst.worst_status[1] == _lib.W_VALUEERROR
        assert np.isnan(got[5, 0]) and status[5, 0] == _lib.W_INDEXERROR and dst.worst_status[0] == _lib.W_INDEXERROR
    assert np.sum(np.isfinite(got)) >= 7 * NW - 6
    # a row range that does not start at 0 overwrites exactly those rows, and grows dst from where it ends
    part = new_series(1, np.full((3, NW, 1), 7.25))
    worst = series.logprob([e.ctx for e in engines], part, code, 2, 4)
    rows = part.read()[:, :, 0]
    assert part.rows == 6 and np.all(rows[:2] == 7.25) and np.array_equal(rows[2:], want[2:6], equal_nan=True)
    assert list(worst) == [max(0, s) if s > 1 else 0 for s in (status[2:6, :2].max(), status[2:6, 2:].max())]
    with pytest.raises(ValueError):
        series.logprob([e.ctx for e in engines], part, code, 7, 1)      # rows past src
    gap = new_series(1)
    with pytest.raises(ValueError):
        series.logprob([e.ctx for e in engines], gap, code, 1, 2)       # row0 past dst's rows
    with pytest.raises(_lib.MsxError):
        series.logprob([e.ctx for e in engines], gap, _lib.MODE_CHISQ, 0, 2)
    assert gap.rows == 0 and part.rows == 6
    for s in (dst, part, gap):
        s.close()


# ---- 2. lincomb, weights, wmoments -----------------------------------------------------------------------------------------
NROWS = 700


def weighted_case():
    """(x series (NROWS, 5, 3), a (ndim 2), b (ndim 1), host arrays): log-densities of a few units' spread with special
    values planted; column 2 of x is constant."""
    if 'reweight_w' not in common._cache:
        rng = np.random.default_rng(23)
        x = np.stack([rng.normal(-300.0, 40.0, (NROWS, NW)), rng.normal(5.0, 1.0, (NROWS, NW)), np.full((NROWS, NW), 0.25)], axis=2)
        a = np.stack([rng.normal(-5e3, 3.0, (NROWS, NW)), rng.normal(0.0, 1.0, (NROWS, NW))], axis=2)
        b = rng.normal(-5e3, 3.0, (NROWS, NW, 1))
        a[3, 0, 0], a[10, 1, 0], a[11, 4, 0], b[12, 2, 0], b[13, 3, 0] = -np.inf, np.nan, np.inf, -np.inf, np.inf
        a[14, 2, 0], b[14, 2, 0] = -np.inf, -np.inf   # (-inf) - (-inf): NaN
        x[3, 0, 0] = np.nan                            # a non-finite value under a zero weight
        common._cache['reweight_w'] = (new_series(3, x, pieces=3), new_series(2, a), new_series(1, b), x, a, b)
    return common._cache['reweight_w']


def test_lincomb_is_numpys_expression():
    from mcmc_spec_amd import _lib
    sx, sa, sb, x, a, b = weighted_case()
    for terms, want in (([(sa, 0, 1.0), (sb, 0, -1.0)], 1.0 * a[:, :, 0] + -1.0 * b[:, :, 0]),
                        ([(sb, 0, 0.625)], 0.625 * b[:, :, 0]),
                        ([(sa, 1, 0.3), (sb, 0, -0.7), (sx, 1, 1e-3), (sa, 0, 0.5)], 0.3 * a[:, :, 1] + -0.7 * b[:, :, 0] + 1e-3 * x[:, :, 1] + 0.5 * a[:, :, 0])):
        dst = rw.log_weights(terms)
        assert dst.rows == NROWS and np.array_equal(dst.read()[:, :, 0], want, equal_nan=True)
        assert np.array_equal(want, rw.lincomb([(t[0].read()[:, :, t[1]], t[2]) for t in terms]), equal_nan=True)
        dst.close()
    dst = new_series(1, np.full((5, NW, 1), 1.5))
    _lib.Series.lincomb([(sa, 1, 2.0), (sb, 0, 1.0)], dst, 3, 10)
    got = dst.read()[:, :, 0]
    assert dst.rows == 13 and np.all(got[:3] == 1.5) and np.array_equal(got[3:], (2.0 * a[:, :, 1] + 1.0 * b[:, :, 0])[3:13])
    for bad in ([(sa, 2, 1.0)], [(sa, 0, 1.0)] * 9, [(sx, 0, 1.0), (dst, 0, 1.0)]):
        with pytest.raises((ValueError, _lib.MsxError)):
            _lib.Series.lincomb(bad, dst, 0, 5)
    with pytest.raises(ValueError):
        _lib.Series.lincomb([(sa, 0, 1.0)], dst, 0, NROWS + 1)
    assert dst.rows == 13 and np.array_equal(dst.read()[:, :, 0], got)
    dst.close()


def logw_of(a, b):
    return 1.0 * a[:, :, 0] + -1.0 * b[:, :, 0]


@pytest.mark.parametrize('n,discard,thin', [(NROWS, 0, 1), (NROWS, 5, 3), (NROWS - 1, 5, 3), (300, 299, 1), (513, 1, 2)])
def test_weights_and_statistics_equal_the_definition(n, discard, thin):
    """(NROWS, 5, 3) and (NROWS - 1, 5, 3) select the same rows; the maximum, however, is taken over rows [0, n)."""
    sx, sa, sb, x, a, b = weighted_case()
    logw = logw_of(a, b)
    ls = rw.log_weights([(sa, 0, 1.0), (sb, 0, -1.0)])
    ws = new_series(1)
    stats = ls.weights(n, ws, discard, thin)
    w = ws.read()[:, :, 0]
    want_w = rw.weights(logw[:n], COUNTS)
    d = ulps(w, want_w)
    print('weights: max ulp distance to np.exp =', int(d.max()), 'over', w.size, 'values')
    assert ws.rows == n and d.max() <= MEASURED_EXP_ULP + 1
    assert np.array_equal(w == 0.0, want_w == 0.0) and w.max() == 1.0
    for i, j in ((3, 0), (10, 1), (11, 4), (12, 2), (13, 3), (14, 2)):
        assert i >= n or w[i, j] == 0.0
    want = rw.weight_stats(logw[:n], w, COUNTS, discard, thin)     # (fed the device's own w: bit for bit)
    for name in ('count', 'nbad', 'nzero', 'sumw', 'sumw2', 'ess'):
        assert np.array_equal(stats[name], want[name]), name
    assert np.all(stats['ess'] > 1.0) and np.all(stats['ess'] < stats['count'])
    # the weighted moments, every column and a subset, with and without the covariance
    for cols in (None, [2, 0]):
        got = sx.wmoments(ws, n, discard, thin, cols)
        ref = rw.wmoments(x[:n], w, COUNTS, discard, thin, cols)
        for name in ('sumw', 'mean', 'cov'):
            assert np.array_equal(got[name], ref[name], equal_nan=True), name
        assert np.array_equal(got['sumw'], stats['sumw'])
        assert np.all(np.isfinite(got['mean']))     # (the NaN at [3, 0, 0] has weight 0: it enters no sum)
        c0, c2 = (0, 2) if cols is None else (1, 0)   # where x's columns 0 and 2 (the constant one) stand
        assert np.allclose(got['mean'][:, c2], 0.25, rtol=1e-15) and np.all(np.abs(got['cov'][:, c2, c2]) < 1e-30)
        assert np.allclose(got['mean'][:, c0], [np.average(f[:, 0][v > 0], weights=v[v > 0]) for f, v in
                                                                   zip(rw.flat(x[:n], COUNTS, discard, thin), rw.flat(w, COUNTS, discard, thin))],
                           rtol=1e-12)
        assert sx.wmoments(ws, n, discard, thin, cols, cov=False)['cov'] is None
    ls.close()
    ws.close()


def test_the_same_selection_and_a_grown_series_give_the_same_bits():
    from mcmc_spec_amd import _lib
    sx, sa, sb, x, a, b = weighted_case()
    logw = logw_of(a, b)
    ref = None
    for cap, pieces in ((0, 1), (0, 7), (4096, 2)):
        ls, xs = new_series(1, logw[:, :, None], pieces=pieces, cap_hint=cap), new_series(3, x, pieces=pieces, cap_hint=cap)
        ws = new_series(1, cap_hint=cap)
        out = []
        for n in (NROWS, NROWS - 1):    # rows 5, 8, .., 698 either way; M differs only if row 699 holds the maximum
            st = ls.weights(n, ws, 5, 3)
            mo = xs.wmoments(ws, n, 5, 3)
            out.append((ws.read(0, NROWS - 1), st, mo))
        if np.array_equal(rw.member_max(logw, COUNTS), rw.member_max(logw[:NROWS - 1], COUNTS)):
            assert np.array_equal(out[0][0], out[1][0])
            assert all(np.array_equal(out[0][1][k], out[1][1][k]) for k in out[0][1])
            assert all(np.array_equal(out[0][2][k], out[1][2][k], equal_nan=True) for k in out[0][2])
        if ref is None:
            ref = out[0]
        assert np.array_equal(out[0][0], ref[0]) and all(np.array_equal(out[0][1][k], ref[1][k]) for k in ref[1])
        assert all(np.array_equal(out[0][2][k], ref[2][k], equal_nan=True) for k in ref[2])
        for s in (ls, xs, ws):
            s.close()
    # a weight that is not zero poisons its column and only its column
    ws = new_series(1, np.ones((NROWS, NW, 1)))
    got = sx.wmoments(ws, NROWS, 0, 1)
    assert np.isnan(got['mean'][0, 0]) and np.all(np.isfinite(got['mean'][0, 1:])) and np.all(np.isfinite(got['mean'][1]))
    assert np.array_equal(got['mean'][1], rw.wmoments(x, np.ones((NROWS, NW)), COUNTS)['mean'][1])
    ws.close()


def test_a_member_without_a_finite_value_and_the_refusals():
    from mcmc_spec_amd import _lib
    logw = np.random.default_rng(4).normal(size=(40, NW))
    logw[:, 2:] = -np.inf
    logw[7, 3] = np.nan
    ls, ws, xs = new_series(1, logw[:, :, None]), new_series(1), new_series(3, np.ones((40, NW, 3)))
    st = ls.weights(40, ws)
    w = ws.read()[:, :, 0]
    assert np.all(w[:, 2:] == 0.0) and st['ess'][1] == 0.0 and st['sumw'][1] == 0.0 and st['nbad'][1] == 1 and st['nzero'][1] == 119
    assert st['ess'][0] > 1.0 and np.array_equal(st['ess'], rw.weight_stats(logw, w, COUNTS)['ess'])
    mo = xs.wmoments(ws, 40)
    assert np.all(np.isnan(mo['mean'][1])) and np.all(mo['mean'][0] == 1.0)
    # W == 0 for a member that is asked for samples: refused, nothing written
    dst = [new_series(3, np.full((2, 1, 3), 9.0), counts=(1,)) for _ in range(2)]
    with pytest.raises(ValueError, match='sum to zero'):
        xs.resample(ws, 40, [5, 5], dst)
    assert [d.rows for d in dst] == [2, 2] and all(np.all(d.read() == 9.0) for d in dst)
    idx = xs.resample(ws, 40, [5, 0], dst)   # ... and not asked: an empty nout
    assert [d.rows for d in dst] == [5, 0] and len(idx[1]) == 0
    neg = new_series(1, -np.ones((40, NW, 1)))
    with pytest.raises(ValueError, match='negative'):
        xs.resample(neg, 40, [5, 0], dst)
    assert [d.rows for d in dst] == [5, 0]
    lib, dp = ls.lib, _lib.dptr
    out = np.empty(64)
    two = new_series(2, np.ones((40, NW, 2)))
    other = new_series(1, np.ones((40, 5, 1)), counts=(5,))
    for bad, code in ((dict(n=41), _lib.MSX_ERR_RANGE), (dict(n=0), _lib.MSX_ERR_RANGE), (dict(n=10, discard=10), _lib.MSX_ERR_RANGE),
                      (dict(thin=0), _lib.MSX_ERR_INVALID), (dict(discard=-1), _lib.MSX_ERR_INVALID), (dict(w=ls), _lib.MSX_ERR_INVALID),
                      (dict(w=two), _lib.MSX_ERR_INVALID), (dict(w=other), _lib.MSX_ERR_INVALID), (dict(src=two), _lib.MSX_ERR_INVALID)):
        kw = dict(src=ls, n=40, discard=0, thin=1, w=ws)
        kw.update(bad)
        assert lib.msx_series_weights(kw['src'].h, kw['n'], kw['discard'], kw['thin'], kw['w'].h, dp(out)) == code, bad
    cols = np.array([0, 3], dtype=np.uint32)
    assert lib.msx_series_wmoments(xs.h, ws.h, 40, 0, 1, _lib.uptr(cols), 2, dp(out), dp(out), None) == _lib.MSX_ERR_RANGE
    assert lib.msx_series_wmoments(xs.h, two.h, 40, 0, 1, None, 3, dp(out), dp(out), None) == _lib.MSX_ERR_INVALID
    assert lib.msx_series_wmoments(xs.h, ws.h, 41, 0, 1, None, 3, dp(out), dp(out), None) == _lib.MSX_ERR_RANGE
    assert ws.rows == 40 and np.array_equal(ws.read()[:, :, 0], w)
    for s in [ls, ws, xs, neg, two, other] + dst:
        s.close()


# ---- 3. msx_series_resample ------------------------------------------------------------------------------------------------
def dyadic(shape, seed, zeros=0.25):
    rng = np.random.default_rng(seed)
    w = rng.integers(0, 1 << 12, size=shape).astype(np.float64) / 1024.0
    w[rng.random(shape) < zeros] = 0.0
    return w


def check_resample(x, w, nout, seed, discard=0, thin=1, exact=False, counts=COUNTS):
    """The device's draw from host rows x (n, nw, ndim) and weights w (n, nw) against the definition; exact: against plain
    NumPy's cumsum / searchsorted as well.  Two calls give the same bits."""
    n = len(x)
    xs, ws = new_series(x.shape[2], x, counts=counts), new_series(1, w[:, :, None], counts=counts)
    dst = [new_series(x.shape[2], counts=(1,)) for _ in counts]
    idx = xs.resample(ws, n, nout, dst, discard, thin, seed)
    want_rows, want_idx = rw.resample(x, ws.read()[:, :, 0], nout, seed, counts, discard, thin)
    fx, fw = rw.flat(x, counts, discard, thin), rw.flat(w, counts, discard, thin)
    for m in range(len(counts)):
        assert dst[m].rows == nout[m] and np.array_equal(idx[m], want_idx[m]), m
        if nout[m] == 0:
            continue
        got = dst[m].read()[:, 0, :]
        assert np.array_equal(got, want_rows[m]) and np.array_equal(got, fx[m][idx[m]])
        assert np.all(fw[m][idx[m]] > 0.0) and np.all(np.diff(idx[m]) >= 0)
        if exact:
            c = np.cumsum(fw[m])
            assert c[-1] < 2.0 ** 40
            t = (np.arange(nout[m]) + rw.u0(seed, m)) * (c[-1] / nout[m])
            assert np.array_equal(idx[m], np.minimum(np.searchsorted(c, t, side='right'), np.nonzero(fw[m] > 0)[0][-1]))
    again = [new_series(x.shape[2], np.zeros((3, 1, x.shape[2])), counts=(1,)) for _ in counts]   # (rows it held are dropped)
    idx2 = xs.resample(ws, n, nout, again, discard, thin, seed)
    for m in range(len(counts)):
        assert np.array_equal(idx2[m], idx[m]) and again[m].rows == nout[m]
        assert nout[m] == 0 or np.array_equal(again[m].read(), dst[m].read())
    other = xs.resample(ws, n, nout, again, discard, thin, seed + 1)
    for s in [xs, ws] + dst + again:
        s.close()
    return idx, other


# rows per member so that N_m = rows * W_m crosses the tile's boundaries: members of 2 and 3 walkers cannot both hit T - 1,
# T, T + 1, so the single-member cases below carry those, and the two-member cases unequal sizes around them
@pytest.mark.parametrize('N', [1, 2, T - 1, T, T + 1, 2 * T + 3])
def test_one_member_at_every_tile_boundary(N):
    x = np.random.default_rng(N).normal(size=(N, 1, 4))
    for nout in (1, N, 2 * N + 1):
        w = dyadic((N, 1), 50 + N)
        w[-1, 0] += 0.5
        check_resample(x, w, [nout], 3, exact=True, counts=(1,))
    w = np.exp(np.random.default_rng(N + 1).normal(0.0, 2.0, size=(N, 1)))
    idx, other = check_resample(x, w, [max(N // 2, 1)], 11, counts=(1,))
    assert N < 3 or not np.array_equal(idx[0], other[0])    # (another seed moves the comb)


@pytest.mark.parametrize('rows,discard,thin', [(1, 0, 1), ((T + 1) // 2 + 1, 0, 1), (T + 5, 3, 2), (2 * T + 3, 0, 3)])
def test_two_members_of_unequal_walker_counts(rows, discard, thin):
    rng = np.random.default_rng(rows)
    x = rng.normal(size=(rows, NW, 6))
    np_rows = len(range(discard, rows, thin))
    wd = dyadic((rows, NW), 7 + rows)
    wd[discard, 0] = wd[discard, 2] = 1.0
    check_resample(x, wd, [np_rows * 2, 17], 5, discard, thin, exact=True)
    check_resample(x, wd, [0, 2 * T + 1], 5, discard, thin, exact=True)           # an empty nout for one member
    check_resample(x, np.exp(rng.normal(0.0, 3.0, size=(rows, NW))), [700, 3 * np_rows], 9, discard, thin)


def test_equal_weights_zero_weights_and_all_weight_on_the_last_sample():
    rows = T // 2 + 9
    x = np.random.default_rng(1).normal(size=(rows, NW, 3))
    idx, _ = check_resample(x, np.ones((rows, NW)), [2 * rows, 3 * rows], 2, exact=True)
    assert np.array_equal(idx[0], np.arange(2 * rows)) and np.array_equal(idx[1], np.arange(3 * rows))   # nout = N: the chain in order
    w = np.zeros((rows, NW))
    w[-1, 1] = w[-1, 4] = 3.0                # all weight on each member's last sample
    idx, _ = check_resample(x, w, [40, 1], 2, exact=True)
    assert np.all(idx[0] == 2 * rows - 1) and np.all(idx[1] == 3 * rows - 1)
    w = np.ones((rows, NW))
    w[::2] = 0.0                             # every other row weighs nothing, the last rows included when rows is odd
    w[-3:] = 0.0
    idx, _ = check_resample(x, w, [5 * rows, 7], 4, exact=True)
    assert np.all((idx[0] // 2) % 2 == 1) and idx[0].max() < 2 * (rows - 3)


def test_more_tiles_than_a_tile_holds_values():
    """N = T^2 + T + 3 samples: more tile sums than any blocked second level of T entries would hold.  Ones with a few dyadic
    spikes: every prefix sum is exact, so the indices are plain NumPy's."""
    N = T * T + T + 3
    w = np.ones((N, 1))
    w[[5, T - 1, T, 77 * T + 1, T * T - 1, T * T, N - 1], 0] = [64.0, 0.5, 0.0, 1024.0, 0.25, 8.0, 0.0]
    x = np.arange(N, dtype=np.float64).reshape(N, 1, 1)
    idx, _ = check_resample(x, w, [4099], 21, exact=True, counts=(1,))
    assert idx[0][-1] >= T * T and 77 * T + 1 in idx[0]


def test_resample_refusals_leave_everything_as_it_was():
    from mcmc_spec_amd import _lib
    x = np.random.default_rng(6).normal(size=(20, NW, 3))
    xs, ws = new_series(3, x), new_series(1, np.ones((20, NW, 1)))
    dst = [new_series(3, np.full((2, 1, 3), 9.0), counts=(1,)) for _ in range(2)]
    wide, two = new_series(4, counts=(1,)), new_series(3, counts=(2,))
    lib = xs.lib

    def call(src=xs, w=ws, n=20, discard=0, thin=1, nout=(4, 4), d=dst):
        arr = (C.c_void_p * len(d))(*[s.h if s is not None else None for s in d])
        return lib.msx_series_resample(src.h, w.h, n, discard, thin, 1, _lib.iptr(np.asarray(nout, dtype=np.int64)), arr, None)

    for bad in (dict(nout=(4, -1)), dict(d=[dst[0], dst[0]]), dict(d=[dst[0], wide]), dict(d=[dst[0], two]), dict(d=[dst[0], None]),
                dict(thin=0), dict(discard=-1), dict(w=xs), dict(d=[dst[0], ws])):
        assert call(**bad) == _lib.MSX_ERR_INVALID, bad
    for bad in (dict(n=21), dict(n=0), dict(n=5, discard=5)):
        assert call(**bad) == _lib.MSX_ERR_RANGE, bad
    assert [d.rows for d in dst] == [2, 2] and all(np.all(d.read() == 9.0) for d in dst)
    assert call() == _lib.MSX_OK and [d.rows for d in dst] == [4, 4]
    for s in [xs, ws, wide, two] + dst:
        s.close()


# ---- 4. the samplers ---------------------------------------------------------------------------------------------------------
def shifted_engine(c, sigmas=0.5, cropped=False):
    """Golden case c -- or its cropped copy, mixed_engines' second member -- staged again under a parallax prior whose mean is
    moved by ``sigmas`` of its width."""
    import copy
    from mcmc_spec_amd.engine import Engine
    key = ('reweight_shifted', c.nspec, sigmas, cropped)
    if key not in common._cache:
        c2 = copy.copy(c)
        c2.prior = list(c.prior)
        c2.prior[-2] = c.prior[-2] + sigmas * c.prior[-1]
        eng = Engine(0)
        eng.stage_specs(c.specs)
        n = len(c.data[0]) // 2 + 37
        kw = dict(data=[np.asarray(c.data[0])[:n], np.asarray(c.data[1])[:n]], err=np.asarray(c.err)[:n]) if cropped else {}
        _stage(eng, c2, **kw)
        common._cache[key] = eng
    return common._cache[key]


def check_against_the_definition(r, chain, counts, lp_new, lp_old, discard=0, thin=1, seed=4):
    """A Reweighted against the definition applied to the downloaded chain and the host log-probabilities."""
    n = len(chain)
    logw = 1.0 * lp_new + -1.0 * lp_old
    assert np.array_equal(r.logw.read(0, n)[:, :, 0], logw)
    w = r.w.read(0, n)[:, :, 0]
    assert ulps(w, rw.weights(logw, counts)).max() <= MEASURED_EXP_ULP + 1
    want = rw.weight_stats(logw, w, counts, discard, thin)
    assert all(np.array_equal(r.stats[k], want[k]) for k in want)
    mo, ref = r.moments(), rw.wmoments(chain, w, counts, discard, thin)
    assert all(np.array_equal(mo[k], ref[k]) for k in ref)
    parts, idx = r.resample(seed=seed, want_indices=True)
    rows, want_idx = rw.resample(chain, w, want['count'], seed, counts, discard, thin)
    for m, p in enumerate(parts):
        assert p.rows == want['count'][m] and np.array_equal(idx[m], want_idx[m]) and np.array_equal(p.read()[:, 0, :], rows[m])
    return parts, want


@pytest.mark.parametrize('autocorr', ['device', 'host'])
def test_the_ensemble_sampler(autocorr):
    from mcmc_spec_amd import summary
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    c, engines = mixed_engines('B')
    eng = engines[0]
    s = DeviceEnsembleSampler(16, 6, eng, seed=5, chunk=7, autocorr=autocorr)
    s.run_mcmc(spread(c, 16, 61, 0.3), 40)
    chain = s.get_chain()
    N = 40 * 16
    # its own engine: log-weights exactly 0 (an evaluation's bits do not depend on the launch), ESS = N, the chain in order
    with s.get_reweighted(eng) as r:
        assert np.all(r.logw.read()[:, :, 0] == 0.0) and np.all(r.w.read()[:, :, 0] == 1.0)
        assert r.stats['ess'][0] == N and r.stats['nbad'][0] == 0 and r.stats['nzero'][0] == 0 and r.stats['count'][0] == N
        (p,) = r.resample(nout=N)
        assert p.rows == N and np.array_equal(p.read()[:, 0, :], chain.reshape(N, 6))
        p.close()
    new = shifted_engine(c)
    for discard, thin in ((0, 1), (6, 3)):
        with s.get_reweighted(new, discard=discard, thin=thin) as r:
            flat = chain.reshape(-1, 6)
            parts, st = check_against_the_definition(r, chain, [16], new.logposterior(flat).reshape(40, 16),
                                                     eng.logposterior(flat).reshape(40, 16), discard, thin)
            assert 1.0 < st['ess'][0] < st['count'][0]
            sm = summary.summary_of(parts[0], parts[0].rows)
            assert sm['count'][0] == st['count'][0] and np.all(np.isfinite(sm['quantiles']))
            # the shifted prior pulls the parallax towards its new mean
            assert r.moments()['mean'][0, 5] > np.mean(rw.flat(chain, [16], discard, thin)[0][:, 5])
            parts[0].close()
    assert np.array_equal(s.get_chain(), chain)


def test_the_group_sampler_and_the_analyses_downstream():
    from mcmc_spec_amd import products, summary
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    from test_gpu_products import engine as products_engine
    c, engines = mixed_engines('B')
    counts = [16, 16]
    grp = TargetGroup(engines[:2])
    s = DeviceGroupSampler(counts, 6, grp, seeds=[7, 8], chunk=16, autocorr='device')
    s.run_mcmc([spread(c, 16, 40 + k, 0.3) for k in range(2)], 40)
    chain = np.concatenate([s.get_chain(k) for k in range(2)], axis=1)
    with s.get_reweighted(engines[:2]) as r:
        assert np.all(r.logw.read()[:, :, 0] == 0.0) and list(r.stats['ess']) == [640.0, 640.0]
        parts = r.resample()
        for k in range(2):
            assert np.array_equal(parts[k].read()[:, 0, :], s.get_chain(k).reshape(-1, 6))
            parts[k].close()
    new = [engines[0], shifted_engine(c, cropped=True)]   # the second target under a shifted parallax prior; the first as it was
    with s.get_reweighted(new, discard=4, thin=2) as r:
        lp_new = np.concatenate([e.logposterior(s.get_chain(k).reshape(-1, 6)).reshape(40, 16) for k, e in enumerate(new)], axis=1)
        lp_old = np.concatenate([e.logposterior(s.get_chain(k).reshape(-1, 6)).reshape(40, 16) for k, e in enumerate(engines[:2])], axis=1)
        parts, st = check_against_the_definition(r, chain, counts, lp_new, lp_old, 4, 2)
        assert st['ess'][0] == st['count'][0] == 288 and 1.0 < st['ess'][1] < 288.0
        sm = summary.summary_of(parts[1], parts[1].rows)
        assert sm['count'][0] == 288 and np.all(np.isfinite(sm['median']))
        # a resampled series is a chain like any other: derived columns with the products' engine
        pe = products_engine('B')
        vals = products.summarize_chain(parts[1], parts[1].rows, [pe], ['kep_contrast'], (0.5,), 0, 1)
        assert vals['count'][0] == 288 and np.all(np.isfinite(vals['quantiles']))
        for p in parts:
            p.close()
    grp.close()


def test_a_ladders_rung_against_the_same_composition():
    c, engines = mixed_engines('B')
    eng, nw, betas = engines[0], 12, [1.0, 0.5, 0.25]
    p0 = inside(eng, c, 3 * nw, 71).reshape(3, nw, 6)
    new = shifted_engine(c)
    for autocorr in ('device', 'host'):
        s = solo_of(eng, nw, 6, betas, 11, autocorr=autocorr)
        s.run_mcmc(p0, 30)
        th = s.get_chain(t=1)
        flat = th.reshape(-1, 6)
        for e_new in (None, new):
            target = eng if e_new is None else e_new
            with s.get_reweighted(e_new, t=1) as r:
                assert r.members == [1] and r.stats['count'][0] == 30 * nw
                logw = (1.0 * target.logposterior(flat) + -1.0 * eng.logprior(flat) + -0.5 * eng.loglikelihood(flat)).reshape(30, nw)
                assert np.array_equal(r.logw.read(0, 30)[:, nw:2 * nw, 0], logw)
                w = r.w.read(0, 30)[:, nw:2 * nw, 0]
                assert ulps(w, rw.weights(logw)).max() <= MEASURED_EXP_ULP + 1
                want = rw.weight_stats(logw, w)
                assert all(np.array_equal(r.stats[k], want[k]) for k in want) and 1.0 < want['ess'][0] < 30 * nw
                assert np.array_equal(r.moments()['mean'][0], rw.wmoments(th, w)['mean'][0])
                (p,), (idx,) = r.resample(nout=100, seed=3, want_indices=True)
                assert np.array_equal(idx, rw.draw(w.reshape(-1), 100, rw.u0(3, 1))) and np.array_equal(p.read()[:, 0, :], flat[idx])
                p.close()


def test_a_rung_of_one_target_of_a_group_ladder():
    """DeviceGroupTemperedSampler.target(k): K T members in one series; rung 1 of target 1 against the composition, on the
    resident series and on the uploaded host chain alike."""
    from mcmc_spec_amd.group import TargetGroup
    from test_gpu_group_tempered import group_of
    c, engines = mixed_engines('B')
    members, counts, T = engines[:2], [12, 14], 2
    betas = [[1.0, 0.5], [1.0, 0.4]]
    p0s = [inside(e, c, T * n, 80 + k).reshape(T, n, 6) for k, (e, n) in enumerate(zip(members, counts))]
    grp = TargetGroup(members)
    new = shifted_engine(c, cropped=True)
    stats = []
    for autocorr in ('device', 'host'):
        s = group_of(grp, counts, 6, betas, [21, 22], autocorr=autocorr)
        s.run_mcmc(p0s, 24)
        v = s.target(1)
        th = v.get_chain(t=1)
        flat = th.reshape(-1, 6)
        logw = (1.0 * new.logposterior(flat) + -1.0 * members[1].logprior(flat) + -0.4 * members[1].loglikelihood(flat)).reshape(24, 14)
        with v.get_reweighted(new, t=1) as r:
            m = r.members[0]
            assert len(r.members) == 1 and m == (3 if autocorr == 'device' else 1)
            lo = sum(r.series.counts[:m])
            assert np.array_equal(r.logw.read(0, 24)[:, lo:lo + 14, 0], logw)
            w = r.w.read(0, 24)[:, lo:lo + 14, 0]
            want = rw.weight_stats(logw, w)
            assert all(np.array_equal(r.stats[k], want[k]) for k in want) and 1.0 < want['ess'][0] < 336.0
            assert np.array_equal(r.moments()['mean'][0], rw.wmoments(th, w)['mean'][0])
            (p,), (idx,) = r.resample(seed=6, want_indices=True)
            assert p.rows == 336 and np.array_equal(idx, rw.draw(w.reshape(-1), 336, rw.u0(6, m)))
            assert np.array_equal(p.read()[:, 0, :], flat[idx])
            p.close()
            stats.append(want['ess'][0])
    assert stats[0] == stats[1]     # the same chain either way: the same effective sample size
    grp.close()
