"""Pareto-smoothed importance sampling (include/msx.h, msx_series_psis): "can I trust these importance
weights?"  Kish's effective sample size (``reweight.Reweighted.stats['ess']``) looks healthy while the variance of the weights
is infinite.  PSIS -- Vehtari, Simpson, Gelman, Yao & Gabry (2024), "Pareto smoothed importance sampling" -- fits a generalised
Pareto distribution to the largest weights by the profile posterior mean of Zhang & Stephens (2009), reports its shape ``khat``
(below about 0.7 the weighted estimates are reliable; above it they are not) and replaces those weights by the fitted
quantiles, which stabilises every weighted number downstream.  The reference project has no counterpart: the algorithm is that
of the two papers.

This module holds

  * the NumPy DEFINITION, float64, written from the papers: ``tail_len``, ``gpd_fit``, ``smooth``, ``series_weights`` -- which
    tests/test_gpu_psis.py holds the device to -- and ``pointwise_stats`` / ``compare``, the PSIS-LOO and WAIC estimates of a
    matrix of pointwise log-likelihood terms (Vehtari, Gelman & Gabry 2017) on the host;
  * the user layer on device series: ``smooth_series`` and ``Smoothed``, what ``reweight.Reweighted.smooth()`` returns; and
    ``loo`` / ``loo_series`` / ``compare``, the pointwise checks of a chain on the device (msx_predictive_pointwise /
    msx_series_pointwise), which the samplers' ``get_loo`` call.

A SHORT TAIL: with ``MIN_TAIL - 1`` = 4 tail samples or fewer nothing is fitted or smoothed, ``khat`` is +inf and the status is
``SHORT_TAIL``.  Constant log-ratios end here (no sample lies strictly above the cutoff), and so does a vector without a finite
value.
"""
import numpy as np

from . import _lib
from . import reweight

TAIL_MAX = _lib.PSIS_TAIL_MAX    # the longest tail the device fits (include/msx.h MSX_PSIS_TAIL_MAX)
MIN_TAIL = _lib.PSIS_MIN_TAIL    # the shortest tail that is fitted
LOG_TINY = _lib.PSIS_LOG_TINY    # log of the smallest normal double: the cutoff's floor
OK, SHORT_TAIL = _lib.PSIS_OK, _lib.PSIS_SHORT_TAIL
KHAT_BAD = 0.7                   # above this the papers call the estimate unreliable


# ---- the definition ---------------------------------------------------------------------------------------------------------
def tail_len(S, reff=1.0):
    """M = ceil(min(S / 5, 3 sqrt(S / reff))): how many of S samples the tail takes.  Computed on the host, once; the device
    is handed the number."""
    S = np.asarray(S, dtype=np.float64)
    out = np.ceil(np.minimum(S / 5.0, 3.0 * np.sqrt(S / np.float64(reff)))).astype(np.int64)
    return out if out.ndim else int(out)


def logsumexp(v):
    """max + log(sum(exp(v - max))); -inf for an empty vector or one of -inf alone."""
    v = np.asarray(v, dtype=np.float64)
    if v.size == 0:
        return -np.inf
    top = np.max(v)
    if top == -np.inf:
        return -np.inf
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        return top + np.log(np.sum(np.exp(v - top)))


def gpd_fit(t):
    """(khat, sigma) of the generalised Pareto distribution fitted to the ascending, non-negative exceedances ``t`` (n,) by
    Zhang & Stephens (2009) as PSIS uses it, with the weakly informative prior khat = (n k + 5) / (n + 10)."""
    t = np.asarray(t, dtype=np.float64)
    n = t.size
    m = 30 + int(np.floor(np.sqrt(n)))
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        i = np.arange(1, m + 1, dtype=np.float64)
        b = 1.0 / t[n - 1] + (1.0 - np.sqrt(m / (i - 0.5))) / (3.0 * t[int(n / 4.0 + 0.5) - 1])
        k = np.mean(np.log1p(-b[:, None] * t[None, :]), axis=1)
        L = n * (np.log(-b / k) - k - 1.0)
        w = 1.0 / np.sum(np.exp(L[None, :] - L[:, None]), axis=1)
        bbar = np.sum(b * w) / np.sum(w)
        kf = np.mean(np.log1p(-bbar * t))
        sigma = -kf / bbar
        khat = (n * kf + 5.0) / (n + 10.0)
    return float(khat), float(sigma)


def gpd_quantiles(n, khat, sigma):
    """sigma expm1(-khat log1p(-p_j)) / khat at p_j = (j + 0.5) / n, j < n (the limit -sigma log1p(-p_j) for |khat| < 1e-30)."""
    l1 = np.log1p(-(np.arange(n, dtype=np.float64) + 0.5) / n)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        return -sigma * l1 if abs(khat) < 1e-30 else sigma * np.expm1(-khat * l1) / khat


def smooth(lr, tail_len):
    """PSIS of the log-ratios ``lr`` (S',) with a tail of ``tail_len`` samples.  NaN and +inf are bad (``reweight.bad``): they
    weigh 0 and do not count in S; -inf weighs 0 and counts.  Returns a dict:

      'lw'      (S',) the smoothed log-weights, normalised to a log-sum-exp of 0 (-inf for a bad or -inf entry);
      'pre'     (S',) the same before the normalisation: lr - max outside the tail, the fitted quantile inside it;
      'khat'    the shape (+inf for a short tail), 'sigma' the scale (NaN then), 'status' OK or SHORT_TAIL;
      'tail'    the tail's indices into ``lr``, ordered by (value, index); 'cutoff' the shifted cutoff; 'S' the samples counted.

    ``tail_len`` must lie in 1 .. S - 1."""
    lr = np.asarray(lr, dtype=np.float64).reshape(-1)
    isbad = reweight.bad(lr)
    valid = np.nonzero(~isbad)[0]
    S, M = int(valid.size), int(tail_len)
    if not 1 <= M <= S - 1:
        raise ValueError('smooth: tail_len must lie in 1 .. S - 1 (S = {} samples that are not NaN or +inf)'.format(S))
    out = {'khat': np.inf, 'sigma': np.nan, 'status': SHORT_TAIL, 'tail': np.zeros(0, dtype=np.int64), 'cutoff': LOG_TINY, 'S': S}
    top = np.max(lr[valid])
    if top == -np.inf:   # nothing finite: every weight is 0
        out['pre'] = out['lw'] = np.full(lr.size, -np.inf)
        return out
    with np.errstate(invalid='ignore'):
        x = np.where(isbad, -np.inf, lr - top)
    cutoff = max(float(np.sort(x[valid])[S - M - 1]), LOG_TINY)
    tail = np.nonzero(~isbad & (x > cutoff))[0]
    tail = tail[np.lexsort((tail, x[tail]))]   # by (value, flat index)
    pre = x.copy()
    out.update(cutoff=cutoff, tail=tail)
    if tail.size >= MIN_TAIL:
        n = int(tail.size)
        khat, sigma = gpd_fit(np.exp(x[tail]) - np.exp(cutoff))
        with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
            pre[tail] = np.minimum(np.log(np.exp(cutoff) + gpd_quantiles(n, khat, sigma)), 0.0)
        out.update(khat=khat, sigma=sigma, status=OK)
    out['pre'] = pre
    with np.errstate(invalid='ignore'):
        out['lw'] = pre - logsumexp(pre)
    return out


def series_weights(logw, tail_lens, counts=None, discard=0, thin=1):
    """msx_series_psis of the log-weights ``logw`` (n, nw) by the definition: per member ``smooth`` of its flat selection.
    Returns {'w', 'lw' (n, nw): the smoothed max-normalised weights (0 on a row outside the selection) and the normalised
    log-weights (-inf there); 'khat' (k,), 'status' (k,), 'ntail' (k,), 'tail' (list of k index arrays), 'stats':
    ``reweight.weight_stats`` of the smoothed weights}."""
    logw = np.asarray(logw, dtype=np.float64)
    off = reweight._offsets(counts, logw.shape[1])
    k = len(off) - 1
    w, lw = np.zeros(logw.shape), np.full(logw.shape, -np.inf)
    rows = np.arange(logw.shape[0])[discard::thin]
    khat, status, tails = np.empty(k), np.empty(k, dtype=np.int64), []
    for m in range(k):
        sel = logw[discard::thin, off[m]:off[m + 1]]
        r = smooth(sel.reshape(-1), np.asarray(tail_lens).reshape(-1)[m])
        with np.errstate(invalid='ignore'):
            top = np.max(r['lw'])
            wm = np.zeros(r['lw'].size) if top == -np.inf else np.exp(r['lw'] - top)
        w[rows, off[m]:off[m + 1]] = wm.reshape(sel.shape)
        lw[rows, off[m]:off[m + 1]] = r['lw'].reshape(sel.shape)
        khat[m], status[m] = r['khat'], r['status']
        tails.append(r['tail'])
    return {'w': w, 'lw': lw, 'khat': khat, 'status': status, 'ntail': np.array([t.size for t in tails], dtype=np.int64), 'tail': tails,
            'stats': reweight.weight_stats(logw, w, counts, discard, thin)}


NAMES = ('lppd', 'p_waic', 'elpd_waic', 'elpd_loo', 'p_loo', 'khat')


def pointwise_stats(ll, reff=1.0):
    """PSIS-LOO and WAIC of the pointwise log-likelihood terms ``ll`` (n_obs, S): observation i under sample s.  Per
    observation (n_obs,): ``lppd`` = logsumexp_s(ll) - log S; ``p_waic`` = var_s(ll, ddof=1), two passes; ``elpd_waic`` = lppd -
    p_waic; PSIS of the ratios -ll_i with a tail of min(tail_len(S, reff), S - 1) gives ``khat`` and ``elpd_loo`` =
    logsumexp_s(lw_s + ll_is) (NaN with fewer than tail + 1 terms that are not NaN or -inf); ``p_loo`` = lppd - elpd_loo.
    'total' holds their sums over i (khat apart), 'se' sqrt(n_obs var_i(., ddof=1)), 'n_bad_k' the count of khat > 0.7."""
    ll = np.asarray(ll, dtype=np.float64)
    if ll.ndim != 2 or ll.shape[1] < 2:
        raise ValueError('pointwise_stats: ll must have shape (n_obs, S), S >= 2')
    n_obs, S = ll.shape
    M = min(tail_len(S, reff), S - 1)
    out = {name: np.empty(n_obs) for name in NAMES}
    for i in range(n_obs):
        row = ll[i]
        with np.errstate(invalid='ignore', over='ignore'):
            out['lppd'][i] = logsumexp(row) - np.log(S)
            mean = np.sum(row) / S
            out['p_waic'][i] = np.sum((row - mean) ** 2) / (S - 1)
            try:
                r = smooth(-row, M)
                out['khat'][i] = r['khat']
                out['elpd_loo'][i] = logsumexp(r['lw'] + row)
            except ValueError:   # fewer than M + 1 terms that are not NaN or -inf: nothing to leave out
                out['khat'][i] = out['elpd_loo'][i] = np.nan
    out['elpd_waic'] = out['lppd'] - out['p_waic']
    out['p_loo'] = out['lppd'] - out['elpd_loo']
    names = NAMES[:5]
    out['total'] = {name: float(np.sum(out[name])) for name in names}
    out['se'] = {name: float(np.sqrt(n_obs * np.var(out[name], ddof=1))) if n_obs > 1 else float('nan') for name in names}
    out['n_bad_k'] = int(np.sum(out['khat'] > KHAT_BAD))
    out['n_obs'] = n_obs
    return out


def compare(a, b):
    """The difference a - b of two ``pointwise_stats`` results on the same observations: {'elpd_loo', 'elpd_waic': (difference of
    the totals, standard error of the pointwise differences)}.  Results whose ``n_obs`` differ are refused."""
    if a['n_obs'] != b['n_obs']:
        raise ValueError('compare: the results cover {} and {} observations'.format(a['n_obs'], b['n_obs']))
    n = a['n_obs']
    out = {'n_obs': n}
    for name in ('elpd_loo', 'elpd_waic'):
        d = np.asarray(a[name]) - np.asarray(b[name])
        out[name] = (float(np.sum(d)), float(np.sqrt(n * np.var(d, ddof=1))) if n > 1 else float('nan'))
    return out


# ---- the user layer: device series ----------------------------------------------------------------------------------------
def smooth_series(logw, n, w_dst, discard=0, thin=1, reff=1.0, lw_dst=None, want_tail=False):
    """PSIS of the log-weights series ``logw`` (ndim 1) over rows[0:n][discard::thin] into the weights series ``w_dst`` (and
    the normalised log-weights into ``lw_dst``) on the device (msx_series_psis).  The tail lengths come from ``tail_len(S,
    reff)`` with S the member's samples that are not NaN or +inf, counted on the device first.  Returns {'khat', 'status',
    'ntail', 'tail_len' (k,), 'stats': msx_series_weights' statistics of the smoothed weights, 'tail': the tails' flat indices
    with ``want_tail``}."""
    plain = logw.weights(n, w_dst, discard, thin)   # the counts; w_dst is overwritten below
    S = plain['count'] - plain['nbad']
    if np.any(S < 2):
        raise ValueError('smooth_series: every member needs two samples that are not NaN or +inf')
    M = np.minimum(tail_len(S, reff), S - 1)
    out = logw.psis(n, M, w_dst, lw_dst, discard, thin, want_tail)
    out['tail_len'] = M
    return out


class Smoothed(reweight.Reweighted):
    """``Reweighted.smooth()``: the chain of a ``Reweighted`` under its Pareto-smoothed weights -- ``stats``, ``moments`` and
    ``resample`` as there, and ``khat``, ``status``, ``ntail`` (one per member answered for).  It owns its weights alone: close
    it before the ``Reweighted`` it came from."""

    def __init__(self, parent, reff=1.0):
        self.series, self.logw, self.n, self.ctx = parent.series, parent.logw, parent.n, parent.ctx
        self.discard, self.thin, self.members = parent.discard, parent.thin, list(parent.members)
        self.reff = float(reff)
        self.w = _lib.Series(self.ctx, self.series.nw, 1, self.series.counts, cap_hint=self.n)
        self._owned = [self.w]
        try:
            full = smooth_series(self.logw, self.n, self.w, self.discard, self.thin, self.reff)
        except Exception:
            self.close()
            raise
        self.stats = {name: v[self.members] for name, v in full['stats'].items()}
        self.khat, self.status, self.ntail = full['khat'][self.members], full['status'][self.members], full['ntail'][self.members]
        if hasattr(parent, 'worst_status'):
            self.worst_status = parent.worst_status


# ---- the user layer: pointwise model checks (msx_predictive_pointwise / msx_series_pointwise) ------------------------------
# WHAT THIS IS: the observations are the likelihood's own terms -- the npix pixels, then the contrast filters, then the
# photometry bands -- with the (nc + np) / npix weighting the reference samples with.  Pixels are coupled through the continuum
# fit and the broadening, so elpd_loo here is a per-term influence and a RELATIVE score between models on identical data, errors
# and pixels (``compare``); it is not an absolute predictive density.
def _loo_result(out, count, tail, shape, wl=None, matrix=None):
    npix, nc, nph = shape
    n_obs = npix + nc + nph
    res = {name: out[i].copy() for i, name in enumerate(NAMES)}
    cut = {'pixels': slice(0, npix), 'contrast': slice(npix, npix + nc), 'phot': slice(npix + nc, n_obs)}
    for part, sl in cut.items():
        res[part] = {name: res[name][sl] for name in NAMES}
    names = NAMES[:5]
    with np.errstate(invalid='ignore'):
        res['total'] = {name: float(np.sum(res[name])) for name in names}
        res['se'] = {name: float(np.sqrt(n_obs * np.var(res[name], ddof=1))) if n_obs > 1 else float('nan') for name in names}
        res['n_bad_k'] = int(np.sum(res['khat'] > KHAT_BAD))
    order = np.argsort(-np.where(np.isnan(res['khat']), np.inf, res['khat']), kind='stable')[:10]
    kinds = ['pixel'] * npix + ['contrast'] * nc + ['phot'] * nph
    starts = {'pixel': 0, 'contrast': npix, 'phot': npix + nc}
    res['worst'] = [{'obs': int(o), 'kind': kinds[o], 'index': int(o) - starts[kinds[o]], 'khat': float(res['khat'][o]),
                     'wavelength': float(np.asarray(wl)[o]) if wl is not None and kinds[o] == 'pixel' else None} for o in order]
    res.update(n_obs=n_obs, count=int(count), tail_len=int(tail))
    if matrix is not None:
        res['pointwise'] = matrix
    return res


def loo(engine, theta, reff=1.0, pointwise=False, scratch_mb=None, wl=None):
    """PSIS-LOO and WAIC of the samples ``theta`` (n, ndim) on ``engine`` (staged problem and products), per observation, on
    the device (msx_predictive_pointwise).  A dict of the per-observation arrays ``lppd``, ``p_waic``, ``elpd_waic``,
    ``elpd_loo``, ``p_loo``, ``khat`` (n_obs,) -- the pixels, then the contrast filters, then the photometry bands; also split
    into ``pixels``, ``contrast`` and ``phot`` --, ``total`` and ``se`` (the sums over the observations and sqrt(n_obs var_i)),
    ``n_bad_k`` (khat > 0.7), ``worst`` (the ten observations of largest khat, with their wavelength given ``wl`` per pixel),
    ``count`` (the samples that could be evaluated: the others are left out), ``tail_len``, ``status`` (n,) and, with
    ``pointwise``, the matrix ``pointwise`` (n_obs, count) of the terms themselves.  These are the terms of the likelihood the
    reference samples, weighting and all: a per-term influence and a relative score between models on identical data
    (``compare``), not an absolute predictive density."""
    from .predictive import _scratch_bytes
    theta = np.atleast_2d(_lib.as_f64(theta))
    out, status, count, tail, mat = engine.ctx.predictive_pointwise(theta, reff, _scratch_bytes(scratch_mb), pointwise)
    res = _loo_result(out, count, tail, engine.ctx.pointwise_nobs(), wl, mat)
    res['status'] = status
    return res


def loo_series(series, n, engines, discard=0, thin=1, reff=1.0, pointwise=False, scratch_mb=None, wl=None):
    """``loo`` over rows[0:n][discard::thin] of the device chain ``series``, member m's walkers flattened in (row, walker)
    order and evaluated with ``engines[m]``: a list of one dict per member (``worst_status`` in place of ``status``).  ``wl``:
    None or one wavelength array per member."""
    from .predictive import _scratch_bytes
    engines = [engines] if not isinstance(engines, (list, tuple)) else list(engines)
    parts, count, tail, worst = series.pointwise([e.ctx for e in engines], int(n), discard, thin, reff, _scratch_bytes(scratch_mb), pointwise)
    res = []
    for m, (out, mat) in enumerate(parts):
        d = _loo_result(out, count[m], tail[m], engines[m].ctx.pointwise_nobs(), None if wl is None else wl[m], mat)
        d['worst_status'] = int(worst[m])
        res.append(d)
    return res


def print_report(res, label=''):
    """The examples' lines for a ``loo`` dict: the totals with their standard errors, the count of khat > 0.7 and the worst
    observations."""
    print('{}PSIS-LOO over {} samples, {} observations (tail {}): elpd_loo {:.6g} +- {:.3g}  p_loo {:.4g}  elpd_waic {:.6g} +- {:.3g}  p_waic {:.4g}'.format(
        label, res['count'], res['n_obs'], res['tail_len'], res['total']['elpd_loo'], res['se']['elpd_loo'], res['total']['p_loo'],
        res['total']['elpd_waic'], res['se']['elpd_waic'], res['total']['p_waic']))
    print('{}  khat > 0.7 at {} of {} observations (one sample cannot stand in for these)'.format(label, res['n_bad_k'], res['n_obs']))
    for w in res['worst'][:5]:
        where = '{} {}'.format(w['kind'], w['index']) if w['wavelength'] is None else '{:.5g} um'.format(w['wavelength'])
        print('{}    khat {:.3f} at {}'.format(label, w['khat'], where))
