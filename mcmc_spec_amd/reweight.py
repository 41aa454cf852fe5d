"""Importance reweighting of a finished chain (include/msx.h, msx_series_logprob / _lincomb / _weights / _wmoments /
_resample): asking one chain another question -- another prior, ``rad_prior`` switched on, a
likelihood term dropped or re-weighted, what a ladder's rung says about the posterior -- without a second run.  The chain's
rows are scored again on the device, the difference of two log-densities is a log-weight, and the weighted chain is
summarised (effective sample size, weighted moments) or resampled into device series that every other analysis takes.

This module holds

  * the NumPy DEFINITION of the four calls that reduce (``lincomb``, ``weights``, ``wmoments``, ``prefix_sums`` /
    ``draw``), in the device's order of operations, which tests/test_gpu_reweight.py holds the device to;
  * the user layer on device series: ``rescore``, ``log_weights``, ``Reweighted``, and ``of_series`` / ``uploaded`` for
    a resident or a host chain (the samplers' ``get_reweighted`` chooses between them: ``stored.StoredChain.reweighted``).

Member m's FLAT sample is ``x[discard:n:thin][:, walkers of m].reshape(-1, ...)``: (row, walker) order, ``get_chain(flat=True)``'s.
"""
import numpy as np

from . import _lib
from .sampler import counter_streams

TILE = _lib.RESAMPLE_TILE   # samples per tile of the prefix scan (include/msx.h MSX_RESAMPLE_TILE)
LANES = 256                 # a workgroup's threads: the stride of a walker's sum, the lanes of a tile
STREAM = 15                 # the counter generator's stream of u0 (the samplers draw from streams 0 .. 14)
MODES = {'logposterior': _lib.MODE_LOGPOST, 'logprior': _lib.MODE_LOGPRIOR, 'loglikelihood': _lib.MODE_LOGLIKE}


# ---- the definition ---------------------------------------------------------------------------------------------------------
def _offsets(counts, nw):
    counts = np.asarray([nw] if counts is None else counts, dtype=np.int64).reshape(-1)
    if counts.sum() != nw or np.any(counts < 1):
        raise ValueError("the members' walker counts do not add up to the walkers")
    return np.concatenate([[0], np.cumsum(counts)])


def walker_sums(v):
    """(nw,): the sum of each column of ``v`` (n', nw) in the device's order -- thread i of 256 adds elements i, i + 256, ...
    one after the other, then the tree that adds entry i + s to entry i for s = 128, 64, .., 1."""
    v = np.asarray(v, dtype=np.float64)
    rounds = -(-v.shape[0] // LANES)
    a = np.zeros((rounds * LANES, v.shape[1]))
    a[:v.shape[0]] = v
    a = a.reshape(rounds, LANES, v.shape[1])
    with np.errstate(invalid='ignore', over='ignore'):
        acc = np.zeros((LANES, v.shape[1]))
        for r in range(rounds):
            acc = acc + a[r]
        s = LANES // 2
        while s > 0:
            acc[:s] = acc[:s] + acc[s:2 * s]
            s //= 2
    return acc[0]


def member_sums(v, off):
    """(k,): ``walker_sums`` added over each member's walkers in walker order, from 0.0."""
    ws = walker_sums(v)
    out = np.zeros(len(off) - 1)
    with np.errstate(invalid='ignore', over='ignore'):
        for m in range(len(off) - 1):
            s = np.float64(0.0)
            for w in range(off[m], off[m + 1]):
                s = s + ws[w]
            out[m] = s
    return out


def lincomb(terms):
    """``coef_0 * x_0 + coef_1 * x_1 + ...`` for ``terms`` = [(array, coef), ...]: every product rounded, then the additions
    in order (msx_series_lincomb)."""
    with np.errstate(invalid='ignore', over='ignore'):
        acc = np.float64(terms[0][1]) * np.asarray(terms[0][0], dtype=np.float64)
        for x, c in terms[1:]:
            acc = acc + np.float64(c) * np.asarray(x, dtype=np.float64)
    return acc


def bad(logw):
    """A log-weight that is NaN or +inf."""
    logw = np.asarray(logw, dtype=np.float64)
    return np.isnan(logw) | (logw == np.inf)


def member_max(logw, counts=None):
    """M (k,): per member the maximum of the values of ``logw`` (n, nw) that are finite or -inf (-inf when there is none)."""
    logw = np.asarray(logw, dtype=np.float64)
    off = _offsets(counts, logw.shape[1])
    ok = np.where(bad(logw), -np.inf, logw)
    return np.array([ok[:, off[m]:off[m + 1]].max() for m in range(len(off) - 1)])


def weights(logw, counts=None):
    """``w = exp(logw - M_m)`` of ``logw`` (n, nw), rows [0, n): a bad value, and every value of a member without a finite
    one, weighs 0 (msx_series_weights; ``np.exp`` stands for the device library's exp)."""
    logw = np.asarray(logw, dtype=np.float64)
    off = _offsets(counts, logw.shape[1])
    M = np.repeat(member_max(logw, counts), np.diff(off))[None, :]
    with np.errstate(invalid='ignore', over='ignore'):
        w = np.exp(logw - M)
    return np.where(bad(logw) | (M == -np.inf), 0.0, w)


def weight_stats(logw, w, counts=None, discard=0, thin=1):
    """msx_series_weights' statistics of the selection rows[discard::thin] of ``logw``, ``w`` (n, nw): {'count', 'nbad',
    'nzero' (k,) ints, 'sumw', 'sumw2', 'ess' (k,)}, the sums in the device's order."""
    logw, w = np.asarray(logw, dtype=np.float64)[discard::thin], np.asarray(w, dtype=np.float64)[discard::thin]
    off = _offsets(counts, w.shape[1])
    b = bad(logw)
    cut = lambda a: np.array([a[:, off[m]:off[m + 1]].sum() for m in range(len(off) - 1)], dtype=np.int64)
    s1, s2 = member_sums(w, off), member_sums(w * w, off)
    with np.errstate(invalid='ignore', divide='ignore'):
        ess = np.where(s2 > 0.0, (s1 * s1) / s2, 0.0)
    return {'count': w.shape[0] * np.diff(off), 'nbad': cut(b), 'nzero': cut(~b & (w == 0.0)), 'sumw': s1, 'sumw2': s2, 'ess': ess}


def wmoments(x, w, counts=None, discard=0, thin=1, cols=None, cov=True):
    """msx_series_wmoments of ``x`` (n, nw, ndim) under ``w`` (n, nw): {'sumw' (k,), 'mean' (k, ncols), 'cov' (k, ncols, ncols)
    or None}.  A sample of zero weight enters no sum."""
    x, w = np.asarray(x, dtype=np.float64)[discard::thin], np.asarray(w, dtype=np.float64)[discard::thin]
    cols = list(range(x.shape[2])) if cols is None else [int(c) for c in cols]
    off = _offsets(counts, w.shape[1])
    k, nc = len(off) - 1, len(cols)
    zero = w == 0.0
    rep = np.diff(off)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        sumw = member_sums(w, off)
        mean = np.stack([member_sums(np.where(zero, 0.0, w * x[:, :, c]), off) for c in cols], axis=1) / sumw[:, None]
        cv = None
        if cov:
            cv = np.empty((k, nc, nc))
            dev = [x[:, :, c] - np.repeat(mean[:, q], rep)[None, :] for q, c in enumerate(cols)]
            for d in range(nc):
                for e in range(d, nc):
                    cv[:, d, e] = cv[:, e, d] = member_sums(np.where(zero, 0.0, w * (dev[d] * dev[e])), off) / sumw
    return {'sumw': sumw, 'mean': mean, 'cov': cv}


def flat(a, counts=None, discard=0, thin=1):
    """The members' flat samples of ``a`` (n, nw, ...): a list of k arrays (N_m, ...) in (row, walker) order."""
    a = np.asarray(a)[discard::thin]
    off = _offsets(counts, a.shape[1])
    return [a[:, off[m]:off[m + 1]].reshape((-1,) + a.shape[2:]) for m in range(len(off) - 1)]


def prefix_sums(v):
    """The inclusive prefix sums C of the flat weights ``v`` (N,) by msx_series_resample's three-phase scan: inside a tile
    of ``TILE`` values lane l of 256 adds its TILE / 256 consecutive values one after the other and the lanes' totals are
    scanned serially (local_i = E_l + s_e); the tiles' sums are scanned serially (B); C_i = B_tile + local_i."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    N = v.size
    ntiles = -(-N // TILE)
    a = np.zeros(ntiles * TILE)
    a[:N] = v
    a = a.reshape(ntiles, LANES, TILE // LANES)
    with np.errstate(invalid='ignore', over='ignore'):
        s = np.add.accumulate(a, axis=2)
        E = np.add.accumulate(np.concatenate([np.zeros((ntiles, 1)), s[:, :, -1]], axis=1), axis=1)
        local = E[:, :LANES, None] + s
        B = np.add.accumulate(np.concatenate([[0.0], E[:, LANES]]))
        C = B[:-1, None, None] + local
    return C.reshape(-1)[:N]


def u0(seed, member):
    """The uniform in [0, 1) that places member ``member``'s comb: the counter generator's stream 15, index 0, with the
    member's number in the iteration's place (``sampler.counter_streams``)."""
    return float(counter_streams(seed, int(member), 1, 2)[2](STREAM, 1)[0, 0])


def draw(v, nout, u):
    """Systematic resampling of the flat weights ``v`` (N,): the indices (nout,) of samples j = 0 .. nout - 1 -- the first i
    with C_i > t_j, t_j = (j + u) * (W / nout) in two roundings, clamped to the last i with v_i > 0."""
    v = np.asarray(v, dtype=np.float64).reshape(-1)
    C = prefix_sums(v)
    if not np.all(v >= 0.0) or not np.isfinite(C[-1]) or not C[-1] > 0.0:
        raise ValueError('the weights must be finite and non-negative with a positive sum')
    nout = int(nout)
    step = C[-1] / np.float64(nout) if nout else np.float64(0.0)
    t = (np.arange(nout, dtype=np.float64) + np.float64(u)) * step
    last = int(np.nonzero(v > 0.0)[0][-1])
    return np.minimum(np.searchsorted(C, t, side='right'), last).astype(np.int64)


def resample(x, w, nout, seed=0, counts=None, discard=0, thin=1):
    """msx_series_resample of ``x`` (n, nw, ndim) under ``w`` (n, nw): (samples, indices), lists of k arrays (nout_m, ndim)
    and (nout_m,)."""
    xs, ws = flat(x, counts, discard, thin), flat(w, counts, discard, thin)
    nout = np.broadcast_to(np.asarray(nout, dtype=np.int64), (len(xs),))
    idx = [draw(ws[m], nout[m], u0(seed, m)) if nout[m] else np.zeros(0, dtype=np.int64) for m in range(len(xs))]
    return [xs[m][idx[m]] for m in range(len(xs))], idx


# ---- the user layer: device series ----------------------------------------------------------------------------------------
def _mode(mode):
    if mode not in MODES:
        raise ValueError("mode must be 'logposterior', 'logprior' or 'loglikelihood'")
    return MODES[mode]


def rescore(series, n, engines, mode='logposterior'):
    """Rows 0 .. n - 1 of ``series`` (a chain: ndim = 2 nspec + 2) scored under ``engines`` -- one staged ``Engine`` per
    member -- in ``mode``: a new series of ndim 1 with the same members (the caller closes it); its ``worst_status`` (k,)
    holds the members' worst sample status.  A rejected sample gives -inf, an error status NaN."""
    engines = list(engines)
    if len(engines) != series.k:
        raise ValueError('rescore: one engine per member ({} members, {} engines)'.format(series.k, len(engines)))
    out = _lib.Series(engines[0].ctx, series.nw, 1, series.counts, cap_hint=int(n))
    try:
        out.worst_status = series.logprob([e.ctx for e in engines], out, _mode(mode), 0, int(n))
    except Exception:
        out.close()
        raise
    return out


def log_weights(terms, ctx=None, n=None):
    """The log-weight ``sum_j coef_j * series_j[col_j]`` of ``terms`` = [(series, col, coef), ...] (1 .. 8 terms with the
    same members) over rows 0 .. n - 1 (None: the fewest rows a term holds), as a new series of ndim 1 on ``ctx``'s device
    (None: the first term's):
    ``lp_new - lp_old``, ``(1 - beta) * ll`` of a ladder's densities, ``+0.5 * chi_contrast`` of a terms series, or any
    mixture."""
    terms = list(terms)
    if not terms:
        raise ValueError('log_weights: at least one term (series, col, coef)')
    n = min(t[0].rows for t in terms) if n is None else int(n)
    first = terms[0][0]
    out = _lib.Series(first.ctx if ctx is None else ctx, first.nw, 1, first.counts, cap_hint=n)
    try:
        _lib.Series.lincomb(terms, out, 0, n)
    except Exception:
        out.close()
        raise
    return out


class Reweighted:
    """A chain ``series`` (rows 0 .. n - 1, the selection rows[0:n][discard::thin]) under the log-weights ``logw`` (a series
    of ndim 1 with the same members): the weights are formed once, on the device.

    ``stats``: {'count', 'nbad', 'nzero', 'sumw', 'sumw2', 'ess'}, each (k,) -- ``ess`` is Kish's (sum w)^2 / sum w^2;
    ``moments(cols)``: the weighted mean and covariance; ``resample(nout, seed)``: one device series per member, which
    ``summary.summary_of``, ``marginals``, ``corner_counts``, ``modes``, ``products.derive`` and ``predictive.check_series``
    take as they take any series.  ``members``: the members it answers for (None: all; a ladder's rung, a group's target).
    ``close()`` frees the weights and whatever ``owned`` names."""

    def __init__(self, series, logw, n, ctx, discard=0, thin=1, members=None, owned=()):
        self.series, self.logw, self.n, self.ctx = series, logw, int(n), ctx
        self.discard, self.thin = int(discard), int(thin)
        self.members = list(range(series.k)) if members is None else [int(m) for m in members]
        self._owned = list(owned)
        self.w = _lib.Series(ctx, series.nw, 1, series.counts, cap_hint=self.n)
        self._owned.append(self.w)
        try:
            full = logw.weights(self.n, self.w, self.discard, self.thin)
        except Exception:
            self.close()
            raise
        self.stats = {name: v[self.members] for name, v in full.items()}

    def moments(self, cols=None, cov=True):
        """{'sumw' (k,), 'mean' (k, ncols), 'cov' (k, ncols, ncols) or None} under the weights (msx_series_wmoments)."""
        out = self.series.wmoments(self.w, self.n, self.discard, self.thin, cols, cov)
        return {name: None if v is None else v[self.members] for name, v in out.items()}

    def resample(self, nout=None, seed=0, want_indices=False):
        """Systematic resampling (msx_series_resample): a list, one device series of one walker per member (the caller
        closes them), holding ``nout`` samples each (None: as many as the member has; an int, or one per member).  With
        ``want_indices`` also the drawn flat indices."""
        count = len(range(self.discard, self.n, self.thin)) * np.asarray(self.series.counts, dtype=np.int64)
        want = count[self.members] if nout is None else np.broadcast_to(np.asarray(nout, dtype=np.int64), (len(self.members),))
        full = np.zeros(self.series.k, dtype=np.int64)
        full[self.members] = want
        dst = [_lib.Series(self.ctx, 1, self.series.ndim) for _ in range(self.series.k)]
        try:
            idx = self.series.resample(self.w, self.n, full, dst, self.discard, self.thin, seed)
        except Exception:
            for s in dst:
                s.close()
            raise
        for m, s in enumerate(dst):
            if m not in self.members:
                s.close()
        out = [dst[m] for m in self.members]
        return (out, [idx[m] for m in self.members]) if want_indices else out

    def smooth(self, reff=1.0):
        """The same chain under the Pareto-smoothed weights (``psis.Smoothed``; msx_series_psis): this object's interface, and
        ``khat`` / ``status`` per member -- khat above about 0.7 says the weights cannot be trusted, whatever ``stats['ess']``
        shows.  ``reff``: the chain's relative efficiency, for the tail's length.  This object and its ``stats`` stay as they
        are; close the result before this."""
        from .psis import Smoothed
        return Smoothed(self, reff)

    def close(self):
        for s in self._owned:
            s.close()
        self._owned = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def of_series(series, n, engines_old, engines_new, ctx=None, mode='logposterior', discard=0, thin=1, members=None, betas=None,
              owned=(), mode_old=None):
    """``Reweighted`` of the chain ``series`` (rows 0 .. n - 1), sampled under ``engines_old`` in ``mode_old`` (None: ``mode``),
    for the density ``mode`` under ``engines_new`` (one staged Engine per member each): both are scored on the device and the
    log-weight is ``lp_new - lp_old``.  ``betas`` (k,) -- a tempered chain, member m sampled from ``lpr + betas[m] * ll`` -- takes the old
    density apart: with one beta b for the members asked for, ``lp_new - lpr_old - b * ll_old``."""
    engines_old, engines_new = list(engines_old), list(engines_new)
    ctx = engines_old[0].ctx if ctx is None else ctx
    parts = list(owned)
    try:
        new = rescore(series, n, engines_new, mode)
        parts.append(new)
        if betas is None:
            old = rescore(series, n, engines_old, mode if mode_old is None else mode_old)
            parts.append(old)
            terms = [(new, 0, 1.0), (old, 0, -1.0)]
        else:
            if mode != 'logposterior':
                raise ValueError("a tempered chain is reweighted to a 'logposterior'")
            b = {float(np.asarray(betas, dtype=np.float64).reshape(-1)[m]) for m in (range(series.k) if members is None else members)}
            if len(b) != 1:
                raise ValueError('one beta for the members asked for: name one rung')
            lpr = rescore(series, n, engines_old, 'logprior')
            parts.append(lpr)
            ll = rescore(series, n, engines_old, 'loglikelihood')
            parts.append(ll)
            terms = [(new, 0, 1.0), (lpr, 0, -1.0), (ll, 0, -b.pop())]
        logw = log_weights(terms, ctx, n)
        parts.append(logw)
        out = Reweighted(series, logw, n, ctx, discard, thin, members, parts)
    except Exception:
        for s in parts:
            s.close()
        raise
    out.worst_status = np.maximum.reduce([np.asarray(t[0].worst_status) for t in terms])[out.members]
    return out


def uploaded(chain, engines_old, engines_new, counts=None, **kw):
    """``of_series`` for a host chain (n, nw, ndim) -- a host sampler's, one loaded from samples.txt --, through a temporary series
    (``summary.uploaded``'s) that the result owns and frees with its ``close()``."""
    from . import summary
    ctx = list(engines_old)[0].ctx
    up = summary.uploaded(chain, ctx, counts)
    return of_series(up.series, up.n, engines_old, engines_new, ctx=ctx, owned=[up.series], **kw)
