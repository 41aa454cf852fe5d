"""GPU: Pareto-smoothed importance sampling of a log-weight series (include/msx.h, msx_series_psis; csrc/psis_kernels.h;
DESIGN.md section 25) against its NumPy definition, mcmc_spec_amd/psis.py.  (1) the tail's membership and order are the
definition's exactly, khat and the normalised log-weights agree to 1e-9 absolute and the statistics to 1e-9 relative -- the
project's bar for a host definition -- at one lane-stride and several, with short tails, ties, constant vectors and NaN / +inf /
-inf entries; where the definition gives +inf, so does the device; (2) the bits do not depend on how the series grew or on its
capacity; (3) msx_series_wmoments and msx_series_resample take the smoothed weights; (4) a refused call leaves every series as
it was."""
import numpy as np
import pytest

import common
from mcmc_spec_amd import psis
from mcmc_spec_amd import reweight as rw
from test_gpu_rhat import series_ctx

pytestmark = pytest.mark.gpu

TOL = 1e-9   # the project's bar for a host definition: absolute on khat and the log-weights, relative on the statistics


def new_series(ndim, rows=None, counts=(1,), pieces=1, cap_hint=0):
    from mcmc_spec_amd import _lib
    s = _lib.Series(series_ctx(), sum(counts), ndim, list(counts), cap_hint=cap_hint)
    if rows is not None:
        for part in np.array_split(np.asarray(rows, dtype=np.float64).reshape(len(rows), sum(counts), ndim), pieces):
            s.append(part)
    return s


def pareto(k, shape, seed):
    return k * np.random.default_rng(seed).exponential(1.0, shape) - 4000.0   # (log-densities' differences lie far from 0)


def cases():
    """name -> (logw (n, nw), counts, tail_len per member or None for the papers' expression, discard, thin)"""
    out = {}
    for S in (24, 64, 257, 1000, 5000):   # one lane-stride of 256 (24, 64), just over one (257), several
        out['one-member-%d' % S] = (pareto(0.5, (S, 1), S), (1,), None, 0, 1)
    mixed = np.concatenate([pareto(0.3, (200, 2), 1), pareto(0.8, (200, 3), 2)], axis=1)
    mixed[3, 0], mixed[77, 1], mixed[5, 3], mixed[150, 4] = np.nan, np.inf, np.nan, np.inf
    mixed[9, 0], mixed[10, 2], mixed[11, 2] = -np.inf, -np.inf, -np.inf
    mixed[20, 3] = -np.nan
    out['members-2-3-special-values'] = (mixed, (2, 3), None, 0, 1)
    rng = np.random.default_rng(3)
    short = rng.normal(-50.0, 1.0, (8, 3))
    out['tail-of-4'] = (short, (3,), [4], 0, 1)
    out['tail-of-5'] = (short, (3,), [5], 0, 1)
    ties = (np.arange(40, dtype=np.float64) * 0.25).reshape(10, 4)
    ties.reshape(-1)[28:33] = ties.reshape(-1)[30]     # the cutoff (rank 31) falls among five equal values
    out['ties-at-the-cutoff'] = (ties, (4,), [8], 0, 1)
    dup = np.concatenate([np.zeros(30), [1.0, 2.0, 2.0, 2.0, 3.0, 3.0, 4.0]])[::-1].reshape(37, 1).copy()
    out['ties-inside-the-tail'] = (dup, (1,), [7], 0, 1)
    out['all-equal'] = (np.full((25, 2), -3.25), (2,), None, 0, 1)
    nothing = np.concatenate([np.full((30, 2), -np.inf), pareto(0.6, (30, 1), 9)], axis=1)
    out['a-member-without-a-finite-value'] = (nothing, (2, 1), None, 0, 1)
    deep = pareto(0.4, (300, 2), 12)
    deep.reshape(-1)[30:] -= 900.0                     # all but 30 weights underflow: the cutoff's rank lies below the floor
    out['values-below-the-floor'] = (deep, (2,), None, 0, 1)
    out['discard-and-thin'] = (np.concatenate([pareto(0.2, (700, 2), 4), pareto(0.9, (700, 3), 5)], axis=1), (2, 3), None, 13, 3)
    return out


CASES = cases()


def tail_lens(logw, counts, given, discard, thin):
    if given is not None:
        return np.asarray(given, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(counts)])
    sel = logw[discard::thin]
    S = np.array([np.sum(~rw.bad(sel[:, off[m]:off[m + 1]])) for m in range(len(counts))])
    return np.minimum(psis.tail_len(S), S - 1)


def run(logw, counts, M, discard, thin, **kw):
    n = logw.shape[0]
    src = new_series(1, logw[:, :, None], counts, **kw)
    w, lw = new_series(1, None, counts), new_series(1, None, counts)
    got = src.psis(n, M, w, lw, discard, thin, want_tail=True)
    got['w'], got['lw'] = w.read()[:, :, 0], lw.read()[:, :, 0]
    for s in (src, w, lw):
        s.close()
    return got


@pytest.mark.parametrize('name', sorted(CASES))
def test_the_device_is_the_definition(name):
    logw, counts, given, discard, thin = CASES[name]
    M = tail_lens(logw, counts, given, discard, thin)
    want = psis.series_weights(logw, M, counts, discard, thin)
    got = run(logw, counts, M, discard, thin)
    # exactly: the status, the tail's members and their order, the zeros and the -inf
    assert np.array_equal(got['status'], want['status']) and np.array_equal(got['ntail'], want['ntail'])
    for m in range(len(counts)):
        assert np.array_equal(got['tail'][m], want['tail'][m]), m
    assert np.array_equal(np.isneginf(got['lw']), np.isneginf(want['lw'])) and not np.any(np.isnan(got['lw']))
    assert np.array_equal(got['w'] == 0.0, want['w'] == 0.0)
    # where the definition gives +inf, the device gives +inf
    inf = np.isinf(want['khat'])
    assert np.array_equal(np.isinf(got['khat']), inf) and np.all(got['khat'][inf] > 0)
    fin = np.isfinite(want['lw'])
    d_k = float(np.max(np.abs(got['khat'][~inf] - want['khat'][~inf]))) if np.any(~inf) else 0.0
    d_lw = float(np.max(np.abs(got['lw'][fin] - want['lw'][fin]))) if np.any(fin) else 0.0
    nz = want['w'] > 0.0
    d_w = float(np.max(np.abs(got['w'][nz] / want['w'][nz] - 1.0))) if np.any(nz) else 0.0
    rel = {}
    for key in ('sumw', 'sumw2', 'ess'):
        den = np.where(want['stats'][key] == 0.0, 1.0, want['stats'][key])
        rel[key] = float(np.max(np.abs(got['stats'][key] - want['stats'][key]) / den))
    print('psis-figures {}: khat {:.3e} lw {:.3e} w(rel) {:.3e} stats(rel) {}'.format(name, d_k, d_lw, d_w, rel))
    assert d_k <= TOL and d_lw <= TOL and d_w <= TOL and all(v <= TOL for v in rel.values())
    for key in ('count', 'nbad', 'nzero'):
        assert np.array_equal(got['stats'][key], want['stats'][key]), key
    # the log-weights' log-sum-exp is 0 for every member that weighs anything; the largest weight is 1
    off = np.concatenate([[0], np.cumsum(counts)])
    for m in range(len(counts)):
        part = got['lw'][discard::thin, off[m]:off[m + 1]]
        if np.any(np.isfinite(part)):
            assert abs(psis.logsumexp(part.reshape(-1))) <= 1e-12
            assert got['w'][discard::thin, off[m]:off[m + 1]].max() == 1.0
    # rows outside the selection weigh nothing
    outside = np.ones(logw.shape[0], dtype=bool)
    outside[discard::thin] = False
    assert np.all(got['w'][outside] == 0.0) and np.all(got['lw'][outside] == -np.inf)


def test_short_and_fitted_tails_are_told_apart():
    four = run(*[CASES['tail-of-4'][i] for i in (0, 1, 2, 3, 4)])
    five = run(*[CASES['tail-of-5'][i] for i in (0, 1, 2, 3, 4)])
    assert four['status'][0] == psis.SHORT_TAIL and four['khat'][0] == np.inf and four['ntail'][0] == 4
    assert five['status'][0] == psis.OK and np.isfinite(five['khat'][0]) and five['ntail'][0] == 5
    flat = run(*[CASES['all-equal'][i] for i in (0, 1)], tail_lens(*CASES['all-equal']), 0, 1)
    assert flat['status'][0] == psis.SHORT_TAIL and flat['khat'][0] == np.inf and flat['ntail'][0] == 0 and np.all(flat['w'] == 1.0)
    # khat orders with the Pareto shape on the device as in the definition
    khat = [run(pareto(k, (5000, 1), 3), (1,), [psis.tail_len(5000)], 0, 1)['khat'][0] for k in (0.2, 0.5, 0.9)]
    assert khat[0] < khat[1] < khat[2] and khat[0] < 0.5 and khat[2] > 0.7


def test_the_bits_do_not_depend_on_growth_or_capacity():
    logw, counts, given, discard, thin = CASES['discard-and-thin']
    M = tail_lens(logw, counts, given, discard, thin)
    a = run(logw, counts, M, discard, thin)
    b = run(logw, counts, M, discard, thin, pieces=5)                  # grown while it was filled
    c = run(logw, counts, M, discard, thin, cap_hint=4096)             # another capacity
    # the same selection out of a longer series
    longer = np.concatenate([logw, pareto(0.5, (300, logw.shape[1]), 6)])
    src = new_series(1, longer[:, :, None], counts, pieces=2)
    w = new_series(1, None, counts)
    d = src.psis(logw.shape[0], M, w, None, discard, thin, want_tail=True)
    d['w'] = w.read()[:, :, 0]
    assert w.rows == logw.shape[0]
    src.close()
    w.close()
    for other in (b, c, d):
        assert np.array_equal(a['khat'], other['khat']) and np.array_equal(a['w'], other['w'])
        assert all(np.array_equal(x, y) for x, y in zip(a['tail'], other['tail']))
        for key in ('sumw', 'sumw2', 'ess'):
            assert np.array_equal(a['stats'][key], other['stats'][key])
    assert np.array_equal(a['lw'], b['lw']) and np.array_equal(a['lw'], c['lw'])


def test_wmoments_resample_and_reweighted_smooth_take_the_smoothed_weights():
    logw, counts, _, discard, thin = CASES['discard-and-thin']
    n, nw = logw.shape
    x = np.random.default_rng(41).normal(3.0, 1.0, (n, nw, 2))
    sx, sl = new_series(2, x, counts), new_series(1, logw[:, :, None], counts)
    with rw.Reweighted(sx, sl, n, series_ctx(), discard, thin) as plain:
        before = {key: v.copy() for key, v in plain.stats.items()}
        with plain.smooth() as sm:
            S = before['count'] - before['nbad']
            want = psis.series_weights(logw, np.minimum(psis.tail_len(S), S - 1), counts, discard, thin)
            assert np.max(np.abs(sm.khat - want['khat'])) <= TOL and np.array_equal(sm.status, want['status'])
            assert np.array_equal(sm.ntail, want['ntail']) and set(sm.stats) == set(plain.stats)
            assert np.all(np.abs(sm.stats['ess'] / want['stats']['ess'] - 1.0) <= TOL)
            # smoothing pulls the largest weights in: the heavy-tailed member gains effective samples
            assert sm.khat[1] > 0.7 > sm.khat[0] and sm.stats['ess'][1] > plain.stats['ess'][1]
            wd = sm.w.read()[:, :, 0]
            mom, ref = sm.moments(), rw.wmoments(x, wd, counts, discard, thin)
            for key in ('sumw', 'mean', 'cov'):
                assert np.array_equal(mom[key], ref[key]), key
            series, idx = sm.resample(nout=[50, 70], seed=5, want_indices=True)
            _, ref_idx = rw.resample(x, wd, [50, 70], 5, counts, discard, thin)
            assert all(np.array_equal(i, j) for i, j in zip(idx, ref_idx)) and [s.rows for s in series] == [50, 70]
            for s in series:
                s.close()
        assert all(np.array_equal(before[key], plain.stats[key]) for key in before)   # the plain weights are untouched
    sx.close()
    sl.close()


def test_refusals_leave_every_series_as_it_was():
    from mcmc_spec_amd import _lib
    logw = pareto(0.5, (60, 3), 8)
    logw[4, 1] = np.nan
    src = new_series(1, logw[:, :, None], (1, 2))
    held = np.full((10, 3, 1), 0.125)
    w, lw = new_series(1, held, (1, 2)), new_series(1, held, (1, 2))
    other = new_series(1, held[:, :2], (1, 1))
    wide = new_series(2, np.zeros((60, 3, 2)), (1, 2))
    ok = [12, 20]
    bad_calls = [
        (ValueError, lambda: src.psis(60, [0, 20], w, lw)),                       # tail_len < 1
        (ValueError, lambda: src.psis(60, [60, 20], w, lw)),                      # tail_len > S - 1 = 59
        (ValueError, lambda: src.psis(60, [12, 119], w, lw)),                     # member 1: S = 119 with its NaN
        (ValueError, lambda: src.psis(60, [12, _lib.PSIS_TAIL_MAX + 1], w, lw)),  # a tail over MSX_PSIS_TAIL_MAX
        (ValueError, lambda: src.psis(61, ok, w, lw)),                            # n past the rows held
        (ValueError, lambda: src.psis(60, ok, w, lw, 60, 1)),                     # an empty selection
        (_lib.MsxError, lambda: src.psis(60, ok, w, lw, 0, 0)),                   # thin < 1
        (_lib.MsxError, lambda: src.psis(60, ok, w, lw, -1, 1)),
        (_lib.MsxError, lambda: src.psis(60, ok, src, lw)),                       # w_dst is the source
        (_lib.MsxError, lambda: src.psis(60, ok, w, w)),                          # lw_dst is w_dst
        (_lib.MsxError, lambda: src.psis(60, ok, other, lw)),                     # other members
        (_lib.MsxError, lambda: wide.psis(60, ok, w, lw)),                        # log-weights of ndim 2
        (ValueError, lambda: src.psis(60, [12], w, lw)),                          # one tail_len per member
    ]
    for exc, call in bad_calls:
        with pytest.raises(exc):
            call()
        assert w.rows == 10 and lw.rows == 10 and src.rows == 60
        assert np.array_equal(w.read(), held) and np.array_equal(lw.read(), held)
        assert np.array_equal(src.read()[:, :, 0], logw, equal_nan=True)
    assert src.psis(60, [12, 118], w, lw)['ntail'][1] <= 118                       # the largest tail member 1 allows
    assert w.rows == 60 and lw.rows == 60
    for s in (src, w, lw, other, wide):
        s.close()
