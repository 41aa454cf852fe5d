"""NumPy restatements the GPU summary tests compare with (mcmc_spec_amd.summary)."""
import numpy as np


def flat_members(rows, n, discard=0, thin=1, counts=None):
    """rows (nrows, nw, ndim) -> per member the flat sample (n' * W_m, ndim) of rows[:n][discard::thin]."""
    x = np.asarray(rows, dtype=float)[:n][discard::thin]
    counts = [x.shape[1]] if counts is None else list(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    return [x[:, off[m]:off[m + 1]].reshape(-1, x.shape[2]) for m in range(len(counts))]


def order_stats(flat, ranks):
    """np.sort(flat)[ranks] (NaN last, as np.sort orders)."""
    return np.sort(np.asarray(flat, dtype=float))[np.asarray(ranks, dtype=int)]


def loop_counts(x, edges):
    """The reference's literal double loop (mft6.py:2046-2049): counts has len(edges) entries, the last one stays 0."""
    count = np.zeros(len(edges))
    for t in x:
        for b in range(len(edges) - 1):
            if edges[b] <= t < edges[b + 1]:
                count[b] += 1
    return count.astype(np.int64)


def reference_counts(x, edges):
    """The loop restated: searchsorted(edges, x, 'right') - 1, indices >= nbins - 1 (and < 0) dropped; length len(edges)."""
    x = np.asarray(x, dtype=float)
    edges = np.asarray(edges, dtype=float)
    idx = np.searchsorted(edges, x[~np.isnan(x)], 'right') - 1
    idx = idx[(idx >= 0) & (idx < len(edges) - 1)]
    return np.bincount(idx, minlength=len(edges)).astype(np.int64)


def numpy_counts(x, edges):
    return np.histogram(np.asarray(x, dtype=float), bins=np.asarray(edges, dtype=float))[0].astype(np.int64)


def numpy_counts2d(x, y, ex, ey):
    return np.histogram2d(np.asarray(x, dtype=float), np.asarray(y, dtype=float), bins=[ex, ey])[0].astype(np.int64)


def chain_like(n, nw, ndim, seed, repeat=0.7, scale=None):
    """Rows in which every walker keeps its previous row with probability ``repeat`` (a rejected move), else draws anew."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, nw, ndim)) * (1.0 if scale is None else scale)
    keep = rng.random((n, nw)) < repeat
    for t in range(1, n):
        x[t][keep[t]] = x[t - 1][keep[t]]
    return x
