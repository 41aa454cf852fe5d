"""Between-walker convergence and plain moments of a chain: split R-hat (Gelman et al. 2013, BDA3 section 11.4) with the
walkers as the chains, and the pooled mean and covariance.  This module is the DEFINITION, in plain
NumPy on a host chain; ``msx_series_moments`` (include/msx.h) computes the same quantities on a device series in a
summation order of its own, and the samplers' ``get_rhat`` / ``get_moments`` use whichever side holds the chain.

A selection ``x`` has shape (n', W, ncols), n' >= 4.  With ``h = n' // 2`` every walker gives two half-chains, rows
``[0, h)`` and ``[n' - h, n')`` (an odd n' leaves the middle row to neither); half-chain ``j = 2 w + half`` of ``J = 2 W``.
Per column ``m_j`` and ``s2_j`` are the half-chain's mean and variance (``ddof=1``), and

    within = mean_j s2_j,    between = var_j m_j (ddof=1; B / h in the book),
    var_plus = ((h - 1) / h) within + between,    rhat = sqrt(var_plus / within).

Special values are IEEE's: a constant column gives 0 / 0 = NaN.  ``counts`` splits the walker axis into members (a group's
targets, a ladder's rungs), each diagnosed on its own.
"""
import numpy as np

MIN_ROWS = 4


def _members(chain, counts):
    x = np.asarray(chain, dtype=np.float64)
    if x.ndim != 3:
        raise ValueError('chain must have shape (rows, walkers, columns)')
    if x.shape[0] < MIN_ROWS:
        raise ValueError('chain too short')
    counts = [x.shape[1]] if counts is None else [int(c) for c in counts]
    if any(c < 1 for c in counts) or sum(counts) != x.shape[1]:
        raise ValueError("the members' walker counts do not add up to the chain's walkers")
    off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    return [x[:, off[m]:off[m + 1]] for m in range(len(counts))]


def split_parts(chain, counts=None):
    """{'within', 'var_plus', 'between', 'rhat'}, each (k, ncols): split R-hat and what it is made of, per member."""
    out = {name: [] for name in ('within', 'var_plus', 'between', 'rhat')}
    for x in _members(chain, counts):
        n, W, nc = x.shape
        h = n // 2
        halves = np.stack([x[:h], x[n - h:]], axis=2)                  # (h, W, 2, ncols): j = 2 w + half
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            m = np.mean(halves, axis=0).reshape(2 * W, nc)
            s2 = np.var(halves, axis=0, ddof=1).reshape(2 * W, nc)
            within = np.mean(s2, axis=0)
            between = np.var(m, axis=0, ddof=1)
            var_plus = (h - 1) / h * within + between
            rhat = np.sqrt(var_plus / within)
        for name, v in (('within', within), ('var_plus', var_plus), ('between', between), ('rhat', rhat)):
            out[name].append(v)
    return {name: np.array(v) for name, v in out.items()}


def split_rhat(chain, counts=None):
    """Split R-hat per column of ``chain`` (n', W, ncols) over its walkers: (ncols,), or (k, ncols) with ``counts``."""
    r = split_parts(chain, counts)['rhat']
    return r[0] if counts is None else r


def moments(chain, counts=None):
    """{'mean' (ncols,), 'cov' (ncols, ncols), 'count'}: the mean and covariance (``ddof=1``) of the pooled sample, all
    n' W values of each column; with ``counts`` per member, the arrays with a leading axis k."""
    mean, cov, count = [], [], []
    for x in _members(chain, counts):
        flat = x.reshape(-1, x.shape[2])
        with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
            mean.append(np.mean(flat, axis=0))
            cov.append(np.atleast_2d(np.cov(flat, rowvar=False)))
        count.append(flat.shape[0])
    out = {'mean': np.array(mean), 'cov': np.array(cov), 'count': np.array(count, dtype=np.int64)}
    return {name: v[0] for name, v in out.items()} if counts is None else out
