"""Posterior modes of a chain: one joint Gaussian mixture over the chain's columns, hard labels per sample, and the
package's summaries applied per mode.  This module is the DEFINITION, in plain NumPy on a host chain;
``msx_series_modes`` and ``msx_series_mode_labels`` (include/msx.h) compute the same quantities on a device series in a
summation order of their own, and the samplers' ``get_modes`` use whichever side holds the chain.

A chain has shape (rows, walkers, ndim); ``counts`` splits the walker axis into members (a group's targets, a ladder's
rungs), each fitted on its own flat sample of the selected columns ``cols`` (d of them, coordinates < ndim, at most
``MAX_DIM``).  Results always carry the member axis k first (k = 1 without ``counts``).

Standardise.  ``z = (x - center) / scale`` with ``center``, ``scale`` the member's pooled mean and ``sqrt(diag cov)`` of
``diagnostics.moments``; a scale that is not finite or not > 0 raises ValueError.  A sample with a non-finite selected value
is BAD: left out of every sum, counted in ``nbad``, labelled 255.  (Such a sample makes the pooled moments and NumPy's
quantiles non-finite too, so a chain that has one needs ``center``, ``scale`` and ``split_at`` from its caller.)

Starts.  One start per selected column c (``nstarts = d``; one start with ``ncomp == 1``): a hard assignment, component =
the number of thresholds <= x_c, thresholds ``np.quantile(column, j / K)``, j = 1 .. K - 1, of the raw column.  The M-step of
that assignment gives the first parameters (iteration 0).

Iteration it = 1, 2, ..  With L_k the Cholesky factor of Sigma_k and y = L_k^-1 (z - mu_k) by forward substitution,

    lp_k = ln w_k - sum ln diag L_k - |y|^2 / 2 - (d / 2) ln 2 pi,
    lse = m + ln sum_k exp(lp_k - m), m = max_k lp_k,      r_k = exp(lp_k - lse),
    w_k = S_k / N, mu_k = sum r_k z / S_k, Sigma_k = sum r_k z z^T / S_k - mu_k mu_k^T + ridge I,   S_k = sum r_k,

N the good samples, ``loglik = sum lse`` (the likelihood of the parameters the iteration STARTED from).  A start stops after
the iteration it >= 2 where ``|loglik - previous| <= tol |loglik|`` (``status`` CONVERGED, that iteration's M-step is kept), or
at ``max_iter`` (MAXITER); ``niter`` is the last iteration run.  An M-step, the first included, that finds a component with
``not S_k >= 1`` is not applied: the start keeps its parameters and freezes with ``status`` COLLAPSED (parameters NaN when it
had none yet).

Result.  Every start is kept; within a start the components are ordered by descending weight, ties by ascending mean of
the first column.  ``best`` is the start with the largest ``loglik`` (NaN last, the lowest index on ties) and
``bic = -2 loglik + p ln N``, ``p = K (1 + d + d (d + 1) / 2) - 1``.
"""
import numpy as np

from . import diagnostics

MAX_DIM = 8        # MSX_MAX_DIM
MODES_MAX = 4      # MSX_MODES_MAX
BAD = 255          # the label of a bad sample
CONVERGED, MAXITER, COLLAPSED = 0, 1, 2
STATUS = ('converged', 'max_iter', 'collapsed')
LN_2PI = float(np.log(2.0 * np.pi))


def _check(ncomp, max_iter, tol, ridge, discard, thin):
    if not 1 <= int(ncomp) <= MODES_MAX:
        raise ValueError('ncomp must lie in 1 .. {}'.format(MODES_MAX))
    if int(max_iter) < 1 or not tol >= 0.0 or not ridge >= 0.0 or int(discard) < 0 or int(thin) < 1:
        raise ValueError('max_iter >= 1, tol >= 0, ridge >= 0, discard >= 0 and thin >= 1 are needed')


def _columns(ndim, cols):
    cols = list(range(ndim)) if cols is None else [int(c) for c in np.atleast_1d(np.asarray(cols, dtype=np.int64))]
    if not 1 <= len(cols) <= MAX_DIM:
        raise ValueError('between 1 and {} columns can be fitted'.format(MAX_DIM))
    if any(c < 0 or c >= ndim for c in cols):
        raise ValueError('a column outside the chain')
    return cols


def _check_scale(scale):
    if not np.all(np.isfinite(scale) & (scale > 0.0)):
        raise ValueError('a column with a zero or non-finite scale cannot be standardised (a constant column, or a '
                         'non-finite sample: pass center, scale and split_at)')


def start_quantiles(ncomp):
    """The quantiles of a start's thresholds: j / K, j = 1 .. K - 1."""
    return np.arange(1, ncomp) / float(ncomp)


def _check_starts(split_col, split_at, k, ncols, ncomp):
    split_col = np.asarray(split_col, dtype=np.int32).reshape(-1)
    split_at = np.asarray(split_at, dtype=np.float64).reshape(k, split_col.size, ncomp - 1)
    if split_col.size < 1 or np.any((split_col < 0) | (split_col >= ncols)):
        raise ValueError('a start names a position outside cols')
    if ncomp > 1 and (not np.all(split_at[..., 1:] >= split_at[..., :-1]) or np.any(np.isnan(split_at))):
        raise ValueError("a start's thresholds must not descend")
    return split_col, np.ascontiguousarray(split_at)


def cholesky_params(weight, mean, cov):
    """(c, L) of one component in standardised units: ``c = ln w - sum ln diag L - (d / 2) ln 2 pi``."""
    d = mean.shape[0]
    with np.errstate(invalid='ignore', divide='ignore'):
        try:
            L = np.linalg.cholesky(cov)
        except np.linalg.LinAlgError:
            L = np.full((d, d), np.nan)
        return np.log(weight) - np.sum(np.log(np.diagonal(L))) - 0.5 * d * LN_2PI, L


def log_terms(z, weight, mean, cov):
    """lp (N, K): every component's ln w_k N(z; mu_k, Sigma_k) at the standardised samples z (N, d)."""
    N, d = z.shape
    lp = np.empty((N, len(weight)))
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        for k in range(len(weight)):
            c, L = cholesky_params(weight[k], mean[k], cov[k])
            v = z - mean[k]
            y = np.empty_like(v)
            for i in range(d):
                y[:, i] = (v[:, i] - y[:, :i] @ L[i, :i]) / L[i, i]
            lp[:, k] = c - 0.5 * np.sum(y * y, axis=1)
    return lp


def _m_step(r, z, N, ridge):
    """(weight, mean, cov) from responsibilities r (N, K), or None when a component holds less than one sample."""
    S0 = np.sum(r, axis=0)
    if not np.all(S0 >= 1.0):
        return None
    mean = (r.T @ z) / S0[:, None]
    d = z.shape[1]
    cov = np.empty((r.shape[1], d, d))
    for k in range(r.shape[1]):
        cov[k] = (z * r[:, k:k + 1]).T @ z / S0[k] - np.outer(mean[k], mean[k]) + ridge * np.eye(d)
    return S0 / N, mean, cov


def _em(z, xs, at, ncomp, max_iter, tol, ridge):
    """One start on the good standardised samples z (N, d): xs the raw start column, at its thresholds."""
    N, d = z.shape
    hard = np.sum(xs[:, None] >= at[None, :], axis=1) if ncomp > 1 else np.zeros(N, dtype=np.int64)
    par = _m_step((hard[:, None] == np.arange(ncomp)[None, :]).astype(np.float64), z, N, ridge)
    out = {'loglik': np.nan, 'niter': 0, 'status': COLLAPSED}
    if par is None:
        par = (np.full(ncomp, np.nan), np.full((ncomp, d), np.nan), np.full((ncomp, d, d), np.nan))
    else:
        prev = None
        for it in range(1, int(max_iter) + 1):
            lp = log_terms(z, *par)
            with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
                m = np.max(lp, axis=1)
                lse = m + np.log(np.sum(np.exp(lp - m[:, None]), axis=1))
                r = np.exp(lp - lse[:, None])
            out['loglik'], out['niter'] = float(np.sum(lse)), it
            new = _m_step(r, z, N, ridge)
            if new is None:
                out['status'] = COLLAPSED
                break
            par = new
            if prev is not None and abs(out['loglik'] - prev) <= tol * abs(out['loglik']):
                out['status'] = CONVERGED
                break
            out['status'] = MAXITER
            prev = out['loglik']
    out['weight'], out['mean'], out['cov'] = par
    return out


def _ordered(weight, mean):
    """The order of a start's components: descending weight, ties by ascending first-column mean (NaN weights last)."""
    idx = list(range(len(weight)))
    key = lambda i: (1, 0.0, 0.0) if np.isnan(weight[i]) else (0, -weight[i], mean[i, 0])
    return np.array(sorted(idx, key=key), dtype=np.int64)


def _best(loglik):
    ll = np.where(np.isnan(loglik), -np.inf, loglik)
    return int(np.argmax(ll))


class ModeFit:
    """What ``fit`` / ``fit_device`` return.  k members, S starts, K components, d columns:

    ``cols`` (d,), ``ncomp``, ``center``, ``scale`` (k, d), ``split_col`` (S,), ``split_at`` (k, S, K - 1);
    ``weight`` (k, S, K); ``mean_z`` (k, S, K, d), ``cov_z`` (k, S, K, d, d) in standardised units; ``mean``, ``cov`` in raw
    units (``center + scale mu``, ``D Sigma D``); ``loglik``, ``bic`` (k, S); ``niter``, ``status`` (k, S) ints
    (``STATUS`` names them); ``count`` (k,) the member's samples, ``nbad`` (k,) the bad ones; ``best`` (k,).
    ``discard``, ``thin``: the selection it was fitted on."""

    def __init__(self, cols, ncomp, center, scale, split_col, split_at, raw, count, nbad, discard, thin):
        self.cols, self.ncomp = np.array(cols, dtype=np.int64), int(ncomp)
        self.center, self.scale = np.array(center, dtype=np.float64), np.array(scale, dtype=np.float64)
        self.split_col, self.split_at = split_col, split_at
        self.count, self.nbad = np.array(count, dtype=np.int64), np.array(nbad, dtype=np.int64)
        self.discard, self.thin = int(discard), int(thin)
        weight, mean, cov = (np.array(raw[name], dtype=np.float64) for name in ('weight', 'mean', 'cov'))
        self.loglik = np.array(raw['loglik'], dtype=np.float64)
        self.niter, self.status = np.array(raw['niter'], dtype=np.int64), np.array(raw['status'], dtype=np.int64)
        k, S = self.loglik.shape
        for m in range(k):
            for s in range(S):
                o = _ordered(weight[m, s], mean[m, s])
                weight[m, s], mean[m, s], cov[m, s] = weight[m, s][o], mean[m, s][o], cov[m, s][o]
        self.weight, self.mean_z, self.cov_z = weight, mean, cov
        sc = self.scale[:, None, None, :]
        self.mean = self.center[:, None, None, :] + sc * mean
        self.cov = cov * sc[..., :, None] * sc[..., None, :]
        d = self.cols.size
        p = self.ncomp * (1 + d + d * (d + 1) // 2) - 1
        self.bic = -2.0 * self.loglik + p * np.log((self.count - self.nbad).astype(np.float64))[:, None]
        self.best = np.array([_best(self.loglik[m]) for m in range(k)], dtype=np.int64)
        self._chain = self._counts = self._series = self._n = self._owned = self._ctx = None

    @property
    def k(self):
        return self.loglik.shape[0]

    def _walkers(self):
        return self._counts if self._series is None else np.asarray(self._series.counts, dtype=np.int64)

    def params(self, start=None):
        """(weight (k, K), mean_z (k, K, d), cov_z (k, K, d, d)) of every member's best start (or of ``start``)."""
        s = self.best if start is None else np.full(self.k, int(start), dtype=np.int64)
        m = np.arange(self.k)
        return self.weight[m, s], self.mean_z[m, s], self.cov_z[m, s]

    def labels(self, start=None):
        """(labels uint8 (rows', walkers), counts (k, K)) of the selection the fit was made on: ``labels`` of this module on
        the host chain, msx_series_mode_labels on the device series."""
        if self._series is not None:
            w, mu, cv = self.params(start)
            return self._series.mode_labels(self._n, self.discard, self.thin, self.cols, self.center, self.scale, w, mu, cv)
        return labels(self, self._chain, self._counts, start)

    def split(self, start=None):
        """Every member's samples by mode, all ndim coordinates, walker ascending then row ascending: a list (k) of lists
        (K) -- of host arrays (count, ndim) for a host fit, of device series (one walker each; the caller closes them)
        for a device fit, filled by msx_series_mode_labels without a download."""
        if self._series is None:
            lab, _ = self.labels(start)
            sel = _selection(self._chain, self.discard, self.thin)
            off = np.concatenate([[0], np.cumsum(self._counts)])
            return [[sel[:, off[m]:off[m + 1]].transpose(1, 0, 2)[lab[:, off[m]:off[m + 1]].T == j] for j in range(self.ncomp)]
                    for m in range(self.k)]
        from . import _lib
        if self._ctx is None:
            raise ValueError('split needs the context of the series: fit_device(..., ctx=...)')
        w, mu, cv = self.params(start)
        dst = [_lib.Series(self._ctx, 1, self._series.ndim) for _ in range(self.k * self.ncomp)]
        try:
            self._series.mode_labels(self._n, self.discard, self.thin, self.cols, self.center, self.scale, w, mu, cv, dst=dst,
                                     want_labels=False)
        except Exception:
            for s in dst:
                s.close()
            raise
        return [dst[m * self.ncomp:(m + 1) * self.ncomp] for m in range(self.k)]

    def summary(self, q=(0.16, 0.5, 0.84), start=None):
        """Per member and mode over ALL coordinates of the chain: {'count' (k, K), 'weight' (k, K), 'min', 'max', 'median'
        (k, K, ndim), 'quantiles' (k, K, ndim, len(q))}; an empty mode's numbers are NaN.  A device fit takes them from
        ``summary.summary_of`` on the modes' series (NumPy's numbers bit for bit), a host fit from NumPy."""
        q = np.atleast_1d(np.asarray(q, dtype=np.float64))
        parts = self.split(start)
        ndim = self._series.ndim if self._series is not None else self._chain.shape[2]
        out = {'count': np.zeros((self.k, self.ncomp), dtype=np.int64), 'weight': self.params(start)[0]}
        for name, tail in (('min', ()), ('max', ()), ('median', ()), ('quantiles', (q.size,))):
            out[name] = np.full((self.k, self.ncomp, ndim) + tail, np.nan)
        try:
            for m in range(self.k):
                for j in range(self.ncomp):
                    part = parts[m][j]
                    if self._series is None:
                        out['count'][m, j] = n = part.shape[0]
                        if n:
                            out['min'][m, j], out['max'][m, j] = part.min(axis=0), part.max(axis=0)
                            out['median'][m, j] = np.median(part, axis=0)
                            out['quantiles'][m, j] = np.quantile(part, q, axis=0).T
                        continue
                    from . import summary
                    out['count'][m, j] = n = part.rows
                    if n:
                        s = summary.summary_of(part, n, q)
                        for name in ('min', 'max', 'median', 'quantiles'):
                            out[name][m, j] = s[name][0]
        finally:
            if self._series is not None:
                for row in parts:
                    for s in row:
                        s.close()
        return out

    def select(self, members):
        """The result restricted to ``members`` (indices): a ladder's rung, a group's target.  Its ``labels``, ``split`` and
        ``summary`` are the full result's, restricted likewise."""
        return _Selected(self, [int(m) for m in members])

    def close(self):
        """Frees the temporary series of ``uploaded`` (a result of ``fit_device`` leaves its caller's series alone)."""
        if self._owned is not None:
            self._owned.close()
            self._owned = self._series = None


class _Selected:
    """``ModeFit.select``: the arrays' member axis cut to ``members``; the work is the full result's."""
    _ARRAYS = ('center', 'scale', 'split_at', 'weight', 'mean_z', 'cov_z', 'mean', 'cov', 'loglik', 'bic', 'niter', 'status',
               'count', 'nbad', 'best')

    def __init__(self, full, members):
        self.full, self.members = full, members
        for name in ('cols', 'ncomp', 'split_col', 'discard', 'thin'):
            setattr(self, name, getattr(full, name))
        for name in self._ARRAYS:
            setattr(self, name, getattr(full, name)[members])

    @property
    def k(self):
        return len(self.members)

    def params(self, start=None):
        return tuple(a[self.members] for a in self.full.params(start))

    def labels(self, start=None):
        lab, cnt = self.full.labels(start)
        off = np.concatenate([[0], np.cumsum(self.full._walkers())])
        return np.concatenate([lab[:, off[m]:off[m + 1]] for m in self.members], axis=1), cnt[self.members]

    def split(self, start=None):
        parts = self.full.split(start)
        for m, row in enumerate(parts):
            if m not in self.members and self.full._series is not None:
                for s in row:
                    s.close()
        return [parts[m] for m in self.members]

    def summary(self, q=(0.16, 0.5, 0.84), start=None):
        return {name: v[self.members] for name, v in self.full.summary(q, start).items()}

    def close(self):
        self.full.close()


def _selection(chain, discard, thin):
    x = np.asarray(chain, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError('chain must have shape (rows, walkers, columns)')
    return x[int(discard)::int(thin)]


def fit(chain, counts=None, cols=None, ncomp=2, max_iter=50, tol=1e-10, ridge=1e-6, discard=0, thin=1, center=None,
        scale=None, split_col=None, split_at=None):
    """The mixture fit of every member of ``chain`` (rows, walkers, ndim) over rows ``[discard::thin]`` -- see the module's
    text -- as a ``ModeFit``.  ``center``, ``scale`` (k, d) and ``split_col`` (S,), ``split_at`` (k, S, K - 1) replace the
    pooled moments and the quantile starts (positions in ``cols`` and raw thresholds)."""
    _check(ncomp, max_iter, tol, ridge, discard, thin)
    sel = _selection(chain, discard, thin)
    cols = _columns(sel.shape[2], cols)
    members = diagnostics._members(sel[:, :, cols], counts)
    k, d = len(members), len(cols)
    if center is None or scale is None:
        mom = diagnostics.moments(sel[:, :, cols], [x.shape[1] for x in members])
        center = mom['mean'] if center is None else center
        scale = np.sqrt(np.diagonal(mom['cov'], axis1=1, axis2=2)) if scale is None else scale
    center, scale = (np.asarray(a, dtype=np.float64).reshape(k, d) for a in (center, scale))
    _check_scale(scale)
    if split_at is None:
        split_col = np.atleast_1d(np.arange(d if ncomp > 1 else 1, dtype=np.int32) if split_col is None else split_col)
        split_at = np.array([[np.quantile(x.reshape(-1, d)[:, c], start_quantiles(ncomp)) for c in split_col]
                             for x in members]).reshape(k, len(split_col), ncomp - 1)
    elif split_col is None:
        raise ValueError('split_at needs split_col')
    split_col, split_at = _check_starts(split_col, split_at, k, d, ncomp)
    raw = {name: [] for name in ('weight', 'mean', 'cov', 'loglik', 'niter', 'status')}
    count, nbad = [], []
    for m, x in enumerate(members):
        flat = x.reshape(-1, d)
        if flat.shape[0] <= ncomp * (d + 1):
            raise ValueError('a member needs more than ncomp (ncols + 1) samples')
        good = np.all(np.isfinite(flat), axis=1)
        count.append(flat.shape[0])
        nbad.append(int(flat.shape[0] - np.sum(good)))
        z = (flat[good] - center[m]) / scale[m]
        outs = [_em(z, flat[good][:, split_col[s]], split_at[m, s], ncomp, max_iter, tol, ridge) for s in range(split_col.size)]
        for name in raw:
            raw[name].append([o[name] for o in outs])
    out = ModeFit(cols, ncomp, center, scale, split_col, split_at, raw, count, nbad, discard, thin)
    out._chain = np.asarray(chain, dtype=np.float64)
    out._counts = np.array([x.shape[1] for x in members], dtype=np.int64)
    return out


def compare(chain, counts=None, **fit_kw):
    """``bic1 - bic2`` (k,) of every member's best one- and two-component fits: positive means two modes."""
    fit_kw.pop('ncomp', None)
    one, two = fit(chain, counts, ncomp=1, **fit_kw), fit(chain, counts, ncomp=2, **fit_kw)
    m = np.arange(one.k)
    return one.bic[m, one.best] - two.bic[m, two.best]


def labels(result, chain, counts=None, start=None):
    """(labels uint8 (rows', walkers), counts (k, K)): ``argmax_k lp_k`` of every sample of ``chain[discard::thin]`` under
    each member's best start of ``result`` (or ``start``), the lowest k on ties, 255 for a bad sample; and how many
    samples each mode got."""
    sel = _selection(chain, result.discard, result.thin)
    members = diagnostics._members(sel[:, :, result.cols], counts)
    w, mu, cv = result.params(start)
    out, cnt = [], np.zeros((len(members), result.ncomp), dtype=np.int64)
    for m, x in enumerate(members):
        flat = x.reshape(-1, x.shape[2])
        good = np.all(np.isfinite(flat), axis=1)
        lab = np.full(flat.shape[0], BAD, dtype=np.uint8)
        lp = log_terms((flat[good] - result.center[m]) / result.scale[m], w[m], mu[m], cv[m])
        lab[good] = np.argmax(np.where(np.isnan(lp), -np.inf, lp), axis=1)
        cnt[m] = np.bincount(lab[good], minlength=result.ncomp)[:result.ncomp]
        out.append(lab.reshape(x.shape[:2]))
    return np.concatenate(out, axis=1), cnt


def label_gaps(result, chain, counts=None, start=None):
    """The gap between every good sample's two largest lp_k, flat per member (a list of k arrays; K >= 2): how far each
    label is from a tie."""
    sel = _selection(chain, result.discard, result.thin)
    w, mu, cv = result.params(start)
    out = []
    for m, x in enumerate(diagnostics._members(sel[:, :, result.cols], counts)):
        flat = x.reshape(-1, x.shape[2])
        flat = flat[np.all(np.isfinite(flat), axis=1)]
        lp = np.sort(log_terms((flat - result.center[m]) / result.scale[m], w[m], mu[m], cv[m]), axis=1)
        out.append(lp[:, -1] - lp[:, -2])
    return out


def print_table(result, names=None, single=None, q=(0.16, 0.5, 0.84)):
    """The table of a fit: per member the best start, and per mode its probability, its samples and the quantiles ``q`` of every
    coordinate of the chain.  ``single``: the one-component fit of the same selection; ``bic1 - bic2`` is then printed too."""
    sm = result.summary(q)
    ndim = sm['median'].shape[2]
    names = ['x{}'.format(i) for i in range(ndim)] if names is None else list(names)
    for m in range(result.k):
        b = int(result.best[m])
        line = 'member {}: best start {} of {} ({}, {} iterations), loglik {:.3f}'.format(
            m, b, result.loglik.shape[1], STATUS[int(result.status[m, b])], int(result.niter[m, b]), result.loglik[m, b])
        if single is not None:
            line += ', bic1 - bic2 = {:.1f}'.format(float(single.bic[m, single.best[m]] - result.bic[m, b]))
        print(line)
        for j in range(result.ncomp):
            print('  mode {}: p = {:.4f} ({} samples)'.format(j, sm['weight'][m, j], int(sm['count'][m, j])))
            for i, nm in enumerate(names):
                print('    {:5s} '.format(nm) + ' / '.join('{:.6g}'.format(v) for v in sm['quantiles'][m, j, i]))


# ---- the device side -------------------------------------------------------------------------------------------------------
def fit_device(series, n, cols=None, ncomp=2, max_iter=50, tol=1e-10, ridge=1e-6, discard=0, thin=1, center=None, scale=None,
               split_col=None, split_at=None, ctx=None):
    """``fit`` of the first ``n`` rows of a device series (a ``_lib.Series``), without a download: ``center`` and ``scale``
    from msx_series_moments, the starts' thresholds from ``summary.quantiles`` (NumPy's, bit for bit), the EM iterations of
    every (member, start) in one msx_series_modes call.  ``ctx``: the series' context, needed by ``split`` / ``summary``."""
    from . import summary
    _check(ncomp, max_iter, tol, ridge, discard, thin)
    cols = _columns(series.ndim, cols)
    k, d = series.k, len(cols)
    if center is None or scale is None:
        mom = series.moments(n, discard, thin, cols, cov=True)
        center = mom['mean'] if center is None else center
        with np.errstate(invalid='ignore'):
            scale = np.sqrt(np.diagonal(mom['cov'], axis1=1, axis2=2)) if scale is None else scale
    center, scale = (np.ascontiguousarray(np.asarray(a, dtype=np.float64).reshape(k, d)) for a in (center, scale))
    _check_scale(scale)
    if split_at is None:
        split_col = np.arange(d if ncomp > 1 else 1, dtype=np.int32) if split_col is None else np.atleast_1d(split_col)
        if ncomp > 1:
            at = summary.quantiles(series, n, start_quantiles(ncomp), [cols[c] for c in split_col], discard, thin)
        else:
            at = np.zeros((k, len(split_col), 0))
        split_at = at
    elif split_col is None:
        raise ValueError('split_at needs split_col')
    split_col, split_at = _check_starts(split_col, split_at, k, d, ncomp)
    raw, nbad = series.modes(n, discard, thin, cols, center, scale, ncomp, split_col, split_at, max_iter, tol, ridge)
    count = len(range(int(discard), int(n), int(thin))) * np.asarray(series.counts, dtype=np.int64)
    out = ModeFit(cols, ncomp, center, scale, split_col, split_at, raw, count, nbad, discard, thin)
    out._series, out._n, out._ctx = series, int(n), ctx
    return out


def uploaded(chain, ctx, counts=None, **fit_kw):
    """``fit_device`` for a host chain (n, nw, ndim) through a temporary series on ``ctx``'s device (``summary.uploaded``'s);
    the result keeps that series for ``split`` / ``summary`` until ``close()`` (or until it is collected)."""
    from . import summary
    up = summary.uploaded(chain, ctx, counts)
    try:
        out = fit_device(up.series, up.n, ctx=ctx, **fit_kw)
    except Exception:
        up.series.close()
        raise
    out._owned = up.series
    return out

