"""One view of a sampler's stored chain, behind every sampler's posterior analyses.

A sampler builds a ``StoredChain`` when an analysis is asked for; the view holds no state of its own.  It answers, once
for all sampler families, where the chain is (a resident ``_lib.Series``, or the host rows -- which go to the NumPy
definition or are uploaded first), how many rows count (the rows CONSUMED, never ``series.rows``: a ``sample()`` loop left
early leaves rows queued past them), what the members are (a group's targets, a ladder's rungs) and which of them the
caller named.  Every method takes the member ``m`` first -- an index among the view's own members, or None for all of them
(the arrays then keep a leading axis, lists stay lists) -- and holds the analysis' length rule, its host / resident / upload
decision and its library call, each once."""
from contextlib import contextmanager

import numpy as np

from .sampler import _autocorr_1d, _check_tau, _device_integrated_time, _integrated_time

MIN_ROWS = 4     # split R-hat, the rank statistics and the autocorrelation time: 'chain too short' below
EMPTY = 'the selection rows[0:n][discard::thin] is empty'


def pick(out, idx):
    """Member ``idx`` (an index: the member axis goes) or members ``idx`` (a list: it stays) of a per-member result: a dict of
    arrays (entries that are None are dropped), a list, an object with ``.select`` (``ModeFit``), or an array."""
    one = np.ndim(idx) == 0
    if isinstance(out, dict):
        return {name: v[idx] for name, v in out.items() if v is not None}
    if hasattr(out, 'select'):
        return out.select([idx] if one else idx)
    if isinstance(out, list):
        return out[idx] if one else [out[i] for i in idx]
    return out[idx]


def _host_tau(x, c):
    """EnsembleSampler.get_autocorr_time's tau (before ``* thin`` and the tol rule) of a chain x (n, nw, ndim): one FFT per
    walker and dimension, the walkers' autocorrelations averaged."""
    n, nw, ndim = x.shape
    f = np.empty((ndim, n))
    for d in range(ndim):
        f[d] = 0.0
        for k in range(nw):
            f[d] += _autocorr_1d(x[:, k, d])
        f[d] /= nw
    return _integrated_time(f, c)


def _host_rank_stats(x, counts, want, q):
    """``_lib.Series.rank_stats``' dict from ``diagnostics`` on the selection x (n', W, ncols)."""
    from . import diagnostics
    out = {}
    if 'rhat' in want:
        out.update(diagnostics.rank_rhat(x, counts))
    for kind in ('bulk', 'tail', 'mean'):
        if kind in want:
            out['ess_' + kind] = diagnostics.ess(x, kind, counts)
    if 'mcse' in want:
        m = diagnostics.mcse(x, q, counts)
        out['mcse_mean'], out['mcse_quantile'] = m['mean'], m['quantiles']
    return out


class StoredChain:
    """``series``: the resident ``_lib.Series``, or None; ``host(members=None)``: the view's own members side by side, (n, W, ndim), or
    those at the positions ``members`` alone (a group then converts only those targets' chains);
    ``n``: the rows consumed; ``counts``: the walkers of each member of ``series`` (of ``host()`` without one), None for one
    member; ``engines``: one staged ``Engine`` per member, None for a sampler not built on one; ``own``: the indices of the
    view's own members among them (None: all); ``device_modes``: ``modes`` runs on the device (the device samplers) or is
    the definition (the host samplers); ``joined``: the host moments of several members come from one call on their joined
    selections (the ladders) or from one call per member (the groups) -- the memory order of a selection of columns decides
    the last bit of NumPy's sums, and each family keeps the bits it has always had."""

    def __init__(self, series, host, n, ndim, counts=None, engines=None, own=None, device_modes=False, joined=False):
        self.series, self.host, self.n, self.ndim = series, host, int(n), int(ndim)
        self.counts = None if counts is None else [int(c) for c in counts]
        self.engines, self.device_modes, self.joined = engines, device_modes, joined
        self.own = list(range(1 if counts is None else len(self.counts))) if own is None else list(own)

    # ---- the four questions -------------------------------------------------------------------------------------------------
    def _need(self, discard, thin, least=MIN_ROWS):
        """The length rule: the rows selected, at least ``least`` of them."""
        nsel = len(range(int(discard), self.n, int(thin)))
        if nsel < least:
            raise ValueError('chain too short' if least > 1 else EMPTY)
        return nsel

    def _need_gpu(self):
        """The context of the view's own engine; a sampler that was not built on one is refused."""
        if self.engines is None:
            raise ValueError('this needs the GPU: build the sampler on a staged Engine')
        return self.engines[self.own[0]].ctx

    @contextmanager
    def resident(self):
        """(series, n): the resident series, or the host rows uploaded for the length of the block."""
        from . import summary
        if self.series is not None:
            yield self.series, self.n
            return
        if self.n < 1:
            raise ValueError(EMPTY)
        with summary.uploaded(self.host(), self._need_gpu(), self.counts) as up:
            yield up

    def _asked(self, m):
        """The members asked for, as positions among the view's own."""
        return list(range(len(self.own))) if m is None else [range(len(self.own))[int(m)]]

    def _of(self, out, m):
        """A per-member result of the series cut to the view's own members, or to the one asked for."""
        return pick(out, self.own if m is None else self.own[int(m)])

    def _fetch(self, js, discard, thin):
        """The host rows [discard::thin] of the members at the positions ``js`` among the view's own, one array (n', W_j, ndim)
        each, from one fetch of those members alone."""
        x = np.asarray(self.host(js))[discard::thin]
        off = np.concatenate([[0], np.cumsum([x.shape[1]] if self.counts is None else [self.counts[self.own[j]] for j in js])]).astype(int)
        return [x[:, off[i]:off[i + 1]] for i in range(len(js))]

    def _host_parts(self, asked, discard, thin, cols=None):
        """The selection of each of the members ``asked``, each taken alone: a ladder's rungs fetched in one piece, a group's
        targets one by one (no copy)."""
        parts = [p for js in ([asked] if self.joined else [[j] for j in asked]) for p in self._fetch(js, discard, thin)]
        return parts if cols is None else [p[:, :, np.asarray(cols, dtype=np.int64).ravel()] for p in parts]

    @staticmethod
    def _side_by_side(parts):
        return np.concatenate(parts, axis=1), [p.shape[1] for p in parts]

    # ---- the analyses ---------------------------------------------------------------------------------------------------------
    def autocorr_time(self, m=None, quiet=False, c=5.0, tol=50.0, discard=0, thin=1):
        """The integrated autocorrelation time (ndim,) or (members, ndim): on a resident series one msx_series_acf call per
        lag tile over all members, otherwise the host's per-walker FFTs; fewer than 4 rows with ``quiet``: NaN."""
        try:
            n = self._need(discard, thin)
        except ValueError:
            if not quiet:
                raise
            return np.full((self.ndim,) if m is not None else (len(self.own), self.ndim), np.nan)
        if self.series is not None:
            tau = self._of(_device_integrated_time(self.series, self.n, c, discard, thin), m)
        else:
            tau = np.array([_host_tau(x, c) for x in self._host_parts(self._asked(m), discard, thin)])
            tau = tau if m is None else tau[0]
        return _check_tau(tau * thin, n, thin, tol, quiet)

    def moments(self, m=None, discard=0, thin=1, cols=None, cov=True, rhat=True):
        """``Series.moments``' dict -- with ``rhat`` 'rhat' and what it is made of, with ``cov`` 'mean', 'cov', 'count' -- from
        the resident series (one msx_series_moments call over all members) or from ``diagnostics`` on the host rows."""
        from . import diagnostics
        self._need(discard, thin)
        if self.series is not None:
            return self._of(self.series.moments(self.n, discard, thin, cols, cov), m)
        parts, outs = self._host_parts(self._asked(m), discard, thin, cols), []
        for group in ([parts] if self.joined else [[p] for p in parts]):
            x, counts = self._side_by_side(group)
            outs.append(diagnostics.split_parts(x, counts) if rhat else {})
            if cov:
                outs[-1].update(diagnostics.moments(x, counts))
        out = {name: np.concatenate([o[name] for o in outs]) for name in outs[0]}
        return out if m is None else pick(out, 0)

    def rank_stats(self, m, want, discard=0, thin=1, cols=None, q=()):
        """``Series.rank_stats``' dict of what ``want`` names, from the resident series or from ``diagnostics`` on the host
        rows."""
        self._need(discard, thin)
        if self.series is not None:
            return self._of(self.series.rank_stats(self.n, discard, thin, cols, q, want), m)
        x, counts = self._side_by_side(self._host_parts(self._asked(m), discard, thin, cols))
        out = _host_rank_stats(x, counts, want, q)
        return out if m is None else pick(out, 0)

    def rank_rhat(self, m=None, discard=0, thin=1, cols=None):
        st = self.rank_stats(m, ('rhat',), discard, thin, cols)
        return {name: st[name] for name in ('bulk', 'folded', 'rhat')}

    def ess(self, m=None, discard=0, thin=1, cols=None, kind='bulk'):
        if kind not in ('bulk', 'tail', 'mean'):
            raise ValueError("kind must be 'bulk', 'tail' or 'mean'")
        return self.rank_stats(m, (kind,), discard, thin, cols)['ess_' + kind]

    def mcse(self, m=None, discard=0, thin=1, cols=None, q=(0.16, 0.5, 0.84)):
        st = self.rank_stats(m, ('mcse',), discard, thin, cols, q)
        return {'mean': st['mcse_mean'], 'quantiles': st['mcse_quantile']}

    def modes(self, m=None, ncomp=2, discard=0, thin=1, cols=None, **fit_kw):
        """The mixture fit as a ``modes.ModeFit``: the definition on the host rows, or -- ``device_modes`` -- ``fit_device`` on
        the resident series or on the uploaded rows, which the result then owns until its ``close()``."""
        from . import modes
        kw = dict(cols=cols, ncomp=ncomp, discard=discard, thin=thin, **fit_kw)
        if not self.device_modes:
            out = modes.fit(self.host(), self.counts, **kw)
        elif self.series is not None:
            out = modes.fit_device(self.series, self.n, ctx=self._need_gpu(), **kw)
        else:
            out = modes.uploaded(self.host(), self._need_gpu(), self.counts, **kw)
        return out if m is None and len(self.own) == out.k else self._of(out, m)

    def summary(self, m=None, q=(0.16, 0.5, 0.84), discard=0, thin=1, cols=None):
        from . import summary
        with self.resident() as (series, n):
            return self._of(summary.summary_of(series, n, q, cols, discard, thin), m)

    def products(self, cols, m=None, q=(0.16, 0.5, 0.84), discard=0, thin=1, indices=None):
        """``summary``'s dict over derived columns.  ``indices``: positions in each member's flat sample -- one array for
        all members or one per member -- taken from the host rows through msx_products_batch, wherever the chain is."""
        from . import products
        self._need_gpu()
        if indices is None:
            with self.resident() as (series, n):
                return self._of(products.summarize_chain(series, n, self.engines, cols, q, discard, thin), m)
        per = [indices] * len(self.own) if np.ndim(indices[0]) == 0 else list(indices)
        if len(per) != len(self.own):
            raise ValueError('indices: one array for all targets or one per target')
        asked, outs = self._asked(m), []
        for j, x in zip(asked, self._fetch(asked, discard, thin)):
            e, flat = self.engines[self.own[j]], x.reshape(-1, self.ndim)
            outs.append(products._summary_of_values(e.ctx, products.evaluate(e, flat[np.asarray(per[j], dtype=np.int64)], cols), q))
        return {name: np.stack([o[name] for o in outs]) for name in outs[0]} if m is None else outs[0]

    def predictive(self, m=None, q=(0.16, 0.5, 0.84), discard=0, thin=1):
        """``predictive.check_series``' list of one dict per member, or the dict of the one asked for."""
        from . import predictive
        self._need_gpu()
        with self.resident() as (series, n):
            return self._of(predictive.check_series(series, n, self.engines, q, discard, thin), m)

    def loo(self, m=None, discard=0, thin=1, reff=1.0):
        """``psis.loo_series``' list of one dict per member, or the dict of the one asked for."""
        from . import psis
        self._need_gpu()
        with self.resident() as (series, n):
            return self._of(psis.loo_series(series, n, self.engines, discard, thin, reff), m)

    def reweighted(self, engines_new, m=None, betas=None, **kw):
        """``reweight.of_series`` of the resident series or of the uploaded rows (which the result then owns until its
        ``close()``) for ``engines_new``, one per own member; the members of the series that are not the view's keep their
        own engine and -- ``betas``, one per own member: a tempered chain -- a beta of one.  ``kw``: ``of_series``' mode,
        mode_old, discard, thin."""
        from . import reweight
        self._need_gpu()
        if self.n < 1:
            raise ValueError(EMPTY)
        new = list(self.engines)
        for i, e in zip(self.own, engines_new):
            new[i] = e
        if betas is not None:
            kw['betas'] = np.ones(len(self.engines))
            kw['betas'][self.own] = betas
        if m is not None:
            kw['members'] = [self.own[int(m)]]
        if self.series is not None:
            return reweight.of_series(self.series, self.n, self.engines, new, **kw)
        return reweight.uploaded(self.host(), self.engines, new, self.counts, **kw)
