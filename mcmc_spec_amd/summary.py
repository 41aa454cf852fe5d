"""Posterior summaries of a chain held on the device (include/msx.h, msx_series_order_stats / _hist / _hist2d; DESIGN.md
section 14): what the reference computes from a finished chain before it draws anything --

  * the per-parameter median, ``np.median(sample, axis=0)`` (mft6.py:2025, :2730);
  * the 16 / 50 / 84 percentiles of ``corner.corner(..., quantiles=[0.16, 0.5, 0.84])`` (:1554, :1595, :1636, :1662);
  * the 75-edge marginal counts of T1, T2, R1, R2 and R2 / R1 its bimodal fits start from (:2033-2073);
  * corner's 50-bin 1-D and 2-D counts

-- for every member of a series in one call.  The device returns selected elements and integer counts, so every number
here equals NumPy's on the flat chain bit for bit.  A ``series`` is a ``_lib.Series``; ``n`` the rows to use (the
selection is rows[0:n][discard::thin]); a column is a coordinate or ``col_ratio(a, b)``."""
import numpy as np

from ._lib import col_ratio  # noqa: F401  (re-exported: the derived column x[a] / x[b])

RULES = ('reference', 'numpy')


def _check_q(q):
    q = np.atleast_1d(np.asarray(q, dtype=np.float64))
    if q.ndim != 1 or q.size < 1 or not np.all((q >= 0.0) & (q <= 1.0)):   # (a NaN fails the comparison too)
        raise ValueError('quantiles must lie in [0, 1]')
    return q


def _cols(series, cols):
    cols = list(range(series.ndim)) if cols is None else [int(c) for c in np.atleast_1d(np.asarray(cols, dtype=np.int64))]
    if not cols:
        raise ValueError('no column named')
    return cols


def _member_sizes(series, n, discard, thin):
    """N_m of every member: the rows of rows[0:n][discard::thin] times the member's walkers."""
    nrows = len(range(int(discard), int(n), int(thin)))
    if nrows < 1:
        raise ValueError('the selection rows[0:n][discard::thin] is empty')
    return nrows * np.asarray(series.counts, dtype=np.int64)


def _lerp(a, b, t):
    """NumPy's interpolation of its default ('linear') quantile method, with its roundings."""
    d = b - a
    r = a + d * t
    r = np.where(t >= 0.5, b - d * (1.0 - t), r)
    return np.where(t == 0.0, a, r)


def _quantile_ranks(big, q):
    """NumPy's virtual index h = (N - 1) q per member: ranks floor(h), min(floor(h) + 1, N - 1) and the weight h - floor(h)."""
    h = (big[:, None] - 1) * q[None, :]
    lo = np.floor(h)
    t = h - lo
    lo = lo.astype(np.int64)
    return lo, np.minimum(lo + 1, big[:, None] - 1), t


def quantiles(series, n, q, cols=None, discard=0, thin=1):
    """``np.quantile(flat, q, axis=0)`` of every member's flat sample, as (k, ncols, len(q)): per member the device
    selects the elements of ranks floor(h) and min(floor(h) + 1, N - 1), h = (N - 1) q, and the host interpolates."""
    q = _check_q(q)
    cols = _cols(series, cols)
    lo, hi, t = _quantile_ranks(_member_sizes(series, n, discard, thin), q)
    vals, _ = series.order_stats(n, discard, thin, cols, np.concatenate([lo, hi], axis=1))
    return _lerp(vals[:, :, :q.size], vals[:, :, q.size:], t[:, None, :])


def _median_ranks(big):
    return np.stack([(big - 1) // 2, big // 2], axis=1)


def _median(vals):
    """np.median of a flat sample from its two middle elements (one element twice when N is odd): their np.mean."""
    return np.where(vals[..., 0] == vals[..., 1], vals[..., 0], (vals[..., 0] + vals[..., 1]) / 2.0)


def medians(series, n, cols=None, discard=0, thin=1):
    """``np.median(flat, axis=0)`` of every member's flat sample, (k, ncols) (mft6.py:2025: the mean of the two middle
    elements, which is not the 0.5 quantile's interpolation in the last bit)."""
    cols = _cols(series, cols)
    vals, _ = series.order_stats(n, discard, thin, cols, _median_ranks(_member_sizes(series, n, discard, thin)))
    return _median(vals)


def extremes(series, n, cols=None, discard=0, thin=1):
    """(min, max, count): (k, ncols), (k, ncols) and (k,) -- ranks 0 and N - 1 of every member's flat sample."""
    cols = _cols(series, cols)
    big = _member_sizes(series, n, discard, thin)
    vals, count = series.order_stats(n, discard, thin, cols, np.stack([np.zeros_like(big), big - 1], axis=1))
    return vals[:, :, 0], vals[:, :, 1], count


def _edges(lo, hi, nedges):
    """(k, ncols, nedges): the scalar call np.linspace(min, max, nedges) of each (its bits; the array form takes another
    path through linspace as soon as one column's step is zero)."""
    out = np.empty(lo.shape + (nedges,))
    for i in np.ndindex(lo.shape):
        out[i] = np.linspace(lo[i], hi[i], nedges)
    return out


def marginals(series, n, cols, nbins=75, rule='reference', discard=0, thin=1):
    """(edges, counts) of every member's columns between the column's own min and max.

    ``rule='reference'``: the reference's statements (mft6.py:2037-2073) -- ``nbins`` EDGES ``np.linspace(min, max,
    nbins)``, bin b counts edges[b] <= x < edges[b + 1], the maximum itself is counted nowhere, and the counts array has
    the reference's length ``nbins`` with a trailing zero (``t1_count``): edges and counts are both (k, ncols, nbins).
    ``rule='numpy'``: ``np.histogram(x, bins=nbins)`` -- edges (k, ncols, nbins + 1), counts (k, ncols, nbins), the
    last bin closed."""
    nbins = int(nbins)
    if rule not in RULES:
        raise ValueError("rule must be 'reference' or 'numpy'")
    if nbins < 2:
        raise ValueError('nbins must be at least 2')
    cols = _cols(series, cols)
    lo, hi, _ = extremes(series, n, cols, discard, thin)
    if rule == 'numpy':
        edges = _edges(lo, hi, nbins + 1)
        return edges, series.hist(n, discard, thin, cols, edges, closed_last=True)
    edges = _edges(lo, hi, nbins)
    counts = series.hist(n, discard, thin, cols, edges, closed_last=False)
    return edges, np.concatenate([counts, np.zeros(counts.shape[:2] + (1,), dtype=counts.dtype)], axis=2)


def corner_counts(series, n, cols, bins=50, discard=0, thin=1):
    """What ``corner.corner(bins=bins)`` histograms: (edges (k, ncols, bins + 1), counts1d (k, ncols, bins), pairs,
    counts2d (k, npairs, bins, bins)) with ``pairs`` the (i, j), i > j, positions in ``cols`` of each panel: x is column
    ``cols[j]``, y column ``cols[i]``, counts2d[..., bx, by] = ``np.histogram2d(x, y, bins=[ex, ey])``.  Edges run from
    each column's min to its max; the last bin is closed."""
    bins = int(bins)
    if not 1 <= bins <= 128:
        raise ValueError('bins must lie in 1 .. 128')
    cols = _cols(series, cols)
    lo, hi, _ = extremes(series, n, cols, discard, thin)
    edges = _edges(lo, hi, bins + 1)
    counts1d = series.hist(n, discard, thin, cols, edges, closed_last=True)
    pairs = [(i, j) for i in range(len(cols)) for j in range(i)]
    if not pairs:
        return edges, counts1d, pairs, np.zeros(counts1d.shape[:1] + (0, bins, bins), dtype=np.int64)
    codes = [(cols[j], cols[i]) for i, j in pairs]
    ex = np.stack([edges[:, j] for _, j in pairs], axis=1)
    ey = np.stack([edges[:, i] for i, _ in pairs], axis=1)
    return edges, counts1d, pairs, series.hist2d(n, discard, thin, codes, ex, ey, closed_last=True)


def summary_of(series, n, q=(0.16, 0.5, 0.84), cols=None, discard=0, thin=1):
    """The samplers' ``get_summary``: {'count' (k,), 'min', 'max', 'median' (k, ncols), 'quantiles' (k, ncols, len(q))},
    from ONE order-statistics call: ranks 0, N - 1, the two middle ones and the two of every quantile."""
    q = _check_q(q)
    cols = _cols(series, cols)
    big = _member_sizes(series, n, discard, thin)
    lo, hi, t = _quantile_ranks(big, q)
    ranks = np.concatenate([np.zeros_like(big)[:, None], big[:, None] - 1, _median_ranks(big), lo, hi], axis=1)
    vals, count = series.order_stats(n, discard, thin, cols, ranks)
    return {'count': count, 'min': vals[:, :, 0], 'max': vals[:, :, 1], 'median': _median(vals[:, :, 2:4]),
            'quantiles': _lerp(vals[:, :, 4:4 + q.size], vals[:, :, 4 + q.size:], t[:, None, :])}


class _Uploaded:
    """A host chain (n, nw, ndim) as a temporary series on ``ctx``'s device."""

    def __init__(self, chain, ctx, counts=None):
        from . import _lib
        chain = _lib.as_f64(chain)
        if chain.ndim != 3 or chain.shape[0] < 1:
            raise ValueError('chain must have shape (n, nwalkers, ndim), n >= 1')
        self.n = chain.shape[0]
        self.series = _lib.Series(ctx, chain.shape[1], chain.shape[2], counts, cap_hint=self.n)
        try:
            self.series.append(chain)
        except Exception:
            self.series.close()
            raise

    def __enter__(self):
        return self.series, self.n

    def __exit__(self, *exc):
        self.series.close()


def uploaded(chain, ctx, counts=None):
    """``with uploaded(chain, ctx) as (series, n):`` -- the functions above for any host chain (n, nw, ndim): a host
    sampler's, one loaded from samples.txt.  ``ctx``: a ``_lib.Context`` (``engine.ctx``); ``counts``: the members'
    walker counts, None for one member."""
    return _Uploaded(chain, ctx, counts)


def summarize(chain, ctx, counts=None, q=(0.16, 0.5, 0.84), cols=None, discard=0, thin=1, marginal=None, corner=None):
    """``summary_of`` for a host chain (n, nw, ndim), through a temporary series.  ``marginal`` / ``corner``: keyword
    dicts for ``marginals`` / ``corner_counts`` (``{'cols': [...], 'nbins': 75, 'rule': 'reference'}``, ``{'cols': [...],
    'bins': 50}``); their results are added under 'marginals' and 'corner'."""
    q = _check_q(q)
    if marginal is not None and (marginal.get('rule', 'reference') not in RULES or int(marginal.get('nbins', 75)) < 2):
        raise ValueError("marginal: rule must be 'reference' or 'numpy', nbins at least 2")
    with uploaded(chain, ctx, counts) as (series, n):
        out = summary_of(series, n, q, cols, discard, thin)
        if marginal is not None:
            out['marginals'] = marginals(series, n, discard=discard, thin=thin, **marginal)
        if corner is not None:
            out['corner'] = corner_counts(series, n, discard=discard, thin=thin, **corner)
        return out
