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


# ---- rank-normalised R-hat, bulk / tail ESS and MCSE (Vehtari, Gelman, Simpson, Carpenter and Buerkner 2021; DESIGN.md
# section 26) ---------------------------------------------------------------------------------------------------------------
# Everything is per member and per column, on the SPLIT POOL of a selection x (n', W): the J = 2 W half-chains of split_parts,
# h = n' // 2 rows each, S = h J values (an odd n' leaves the middle row out of everything).  A column with a non-finite value
# or with one distinct value gives NaN for every statistic; so does a transformed pool (the folded values) under the same rule.
# The device computes the same quantities (msx_series_split_transform, msx_series_chain_acov; ``_lib.Series.rank_stats``):
# ranks are integers there as here, ndtri evaluates the coefficients below in the same order, and ``geyer_tau`` is shared.

_AS241_A = (3.3871328727963666080e0, 1.3314166789178437745e+2, 1.9715909503065514427e+3, 1.3731693765509461125e+4,
            4.5921953931549871457e+4, 6.7265770927008700853e+4, 3.3430575583588128105e+4, 2.5090809287301226727e+3)
_AS241_B = (1.0, 4.2313330701600911252e+1, 6.8718700749205790830e+2, 5.3941960214247511077e+3, 2.1213794301586595867e+4,
            3.9307895800092710610e+4, 2.8729085735721942674e+4, 5.2264952788528545610e+3)
_AS241_C = (1.42343711074968357734e0, 4.63033784615654529590e0, 5.76949722146069140550e0, 3.64784832476320460504e0,
            1.27045825245236838258e0, 2.41780725177450611770e-1, 2.27238449892691845833e-2, 7.74545014278341407640e-4)
_AS241_D = (1.0, 2.05319162663775882187e0, 1.67638483018380384940e0, 6.89767334985100004550e-1, 1.48103976427480074590e-1,
            1.51986665636164571966e-2, 5.47593808499534494600e-4, 1.05075007164441684324e-9)
_AS241_E = (6.65790464350110377720e0, 5.46378491116411436990e0, 1.78482653991729133580e0, 2.96560571828504891230e-1,
            2.65321895265761230930e-2, 1.24266094738807843860e-3, 2.71155556874348757815e-5, 2.01033439929228813265e-7)
_AS241_F = (1.0, 5.99832206555887937690e-1, 1.36929880922735805310e-1, 1.48753612908506148525e-2, 7.86869131145613259100e-4,
            1.84631831751005468180e-5, 1.42151175831644588870e-7, 2.04426310338993978564e-15)


def _horner(c, r):
    """((c7 r + c6) r + ...) r + c0, each step one multiplication and one addition (no fused operation)."""
    v = np.full_like(r, c[7])
    for i in range(6, -1, -1):
        v = v * r + c[i]
    return v


def ndtri(p):
    """The normal quantile of p in (0, 1): Wichura's algorithm AS 241, PPND16, in float64 ``+ - * /``, ``np.log`` and
    ``np.sqrt``.  0 and 1 give -inf and +inf, anything else outside (0, 1) NaN."""
    p = np.asarray(p, dtype=np.float64)
    out = np.full(p.shape, np.nan)
    q = p - 0.5
    with np.errstate(invalid='ignore', divide='ignore'):
        mid = np.abs(q) <= 0.425
        r = 0.180625 - q[mid] * q[mid]
        out[mid] = q[mid] * _horner(_AS241_A, r) / _horner(_AS241_B, r)
        tail = ~mid & (p > 0.0) & (p < 1.0)
        qt = q[tail]
        r = np.sqrt(-np.log(np.where(qt < 0.0, p[tail], 1.0 - p[tail])))
        near = r <= 5.0
        v = np.empty_like(r)
        rn, rf = r[near] - 1.6, r[~near] - 5.0
        v[near] = _horner(_AS241_C, rn) / _horner(_AS241_D, rn)
        v[~near] = _horner(_AS241_E, rf) / _horner(_AS241_F, rf)
        out[tail] = np.where(qt < 0.0, -v, v)
    out[p == 0.0] = -np.inf
    out[p == 1.0] = np.inf
    return out


def average_ranks(v):
    """1-based ranks of the flat array v, ties sharing the mean of their positions (``scipy.stats.rankdata(v,
    method='average')``); -0.0 and +0.0 tie.  Twice a rank is an integer."""
    v = np.asarray(v, dtype=np.float64).ravel() + 0.0          # (-0.0 + 0.0 = +0.0)
    order = np.argsort(v, kind='stable')
    s = v[order]
    start = np.flatnonzero(np.concatenate([[True], s[1:] != s[:-1]]))
    end = np.concatenate([start[1:], [s.size]])
    twice = np.repeat(start + end + 1, end - start)             # positions start + 1 .. end: mean (start + 1 + end) / 2
    r = np.empty(s.size)
    r[order] = twice / 2.0
    return r


def split_pool(x):
    """(h, J) the half-chains of one member's column x (n', W): column j = 2 w + half, split_parts' order."""
    n, W = x.shape
    h = n // 2
    return np.stack([x[:h], x[n - h:]], axis=2).reshape(h, 2 * W)


def rank_normalize(pool):
    """z = ndtri((r - 3/8) / (S + 1/4)) over the pool (h, J), r its average ranks; all NaN when the pool holds a
    non-finite value or one distinct value."""
    S = pool.size
    if not np.all(np.isfinite(pool)) or np.all(pool == pool.flat[0]):
        return np.full(pool.shape, np.nan)
    r = average_ranks(pool)
    return ndtri((r - 0.375) / (S + 0.25)).reshape(pool.shape)


def _rhat_of(y):
    """The split-R-hat formula of split_parts on ready half-chains y (h, J)."""
    h = y.shape[0]
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        within = np.mean(np.var(y, axis=0, ddof=1))
        between = np.var(np.mean(y, axis=0), ddof=1)
        return np.sqrt(((h - 1) / h * within + between) / within)


def chain_acov(y):
    """(A (h,), mean_var, between) of the chains y (h, J): A(t) = mean_j (1/h) sum_{i < h-t} (y_i - m_j)(y_{i+t} - m_j),
    mean_var = A(0) h / (h - 1), between = var_j(m_j, ddof=1)."""
    h, J = y.shape
    with np.errstate(invalid='ignore', over='ignore'):
        m = np.mean(y, axis=0)
        d = y - m
        nfft = 1 << int(np.ceil(np.log2(max(2 * h, 2))))
        f = np.fft.rfft(d, n=nfft, axis=0)
        ac = np.fft.irfft(f * np.conjugate(f), n=nfft, axis=0)[:h] / h
        ac[0] = np.sum(d * d, axis=0) / h                       # (lag 0 by the direct sum: a constant chain gives exactly 0)
        A = np.mean(ac, axis=1)
        return A, A[0] * h / (h - 1), np.var(m, ddof=1)


def geyer_tau(A, mean_var, between, h, S):
    """(tau, max_t) from the chain-averaged autocovariance A(0 .. L-1), L <= h: Geyer's initial positive and initial
    monotone sequences, as Stan applies them; (None, None) when the prefix ends before the positive sequence does (the caller
    asks for more lags; L == h always decides).  tau >= 1 / log10(S)."""
    if not (np.isfinite(mean_var) and np.isfinite(between)) or not np.all(np.isfinite(A[:2])):
        return np.nan, 0
    L = len(A)
    var_plus = mean_var * (h - 1) / h + between
    if not var_plus > 0.0:                                      # (a spread that underflows: no autocorrelation to speak of)
        return np.nan, 0
    rho = np.zeros(h + 2)

    def r(t):
        return 1.0 - (mean_var - A[t]) / var_plus

    rho_even, rho_odd = 1.0, r(1)
    rho[0], rho[1] = rho_even, rho_odd
    t = 1
    while t < h - 3 and rho_even + rho_odd > 0.0:
        if t + 2 >= L:
            return None, None
        rho_even, rho_odd = r(t + 1), r(t + 2)
        if not (np.isfinite(rho_even) and np.isfinite(rho_odd)):
            return np.nan, 0
        if rho_even + rho_odd >= 0.0:
            rho[t + 1], rho[t + 2] = rho_even, rho_odd
        t += 2
    max_t = t - 2
    if rho_even > 0.0:
        rho[max_t + 1] = rho_even
    for u in range(1, max_t - 1, 2):                            # t = 1, 3, ... <= max_t - 2
        if rho[u + 1] + rho[u + 2] > rho[u - 1] + rho[u]:
            rho[u + 1] = (rho[u - 1] + rho[u]) / 2.0
            rho[u + 2] = rho[u + 1]
    tau = -1.0 + 2.0 * float(np.sum(rho[:max_t + 1])) + rho[max_t + 1]
    return max(tau, 1.0 / np.log10(S)), max_t


def ess_of(y):
    """S / tau of the chains y (h, J): NaN for a pool that is not finite or is constant."""
    h, J = y.shape
    if not np.all(np.isfinite(y)) or np.all(y == y.flat[0]):
        return np.nan
    A, mean_var, between = chain_acov(y)
    tau, _ = geyer_tau(A, mean_var, between, h, h * J)
    return h * J / tau


def _bad(pool):
    return not np.all(np.isfinite(pool)) or bool(np.all(pool == pool.flat[0]))


def _per_column(chain, counts, fn, shape=()):
    """fn(pool (h, J)) for every member and column -> (k, ncols) + shape."""
    members = _members(chain, counts)
    out = np.empty((len(members), members[0].shape[2]) + shape)
    for m, x in enumerate(members):
        for c in range(x.shape[2]):
            out[m, c] = fn(split_pool(x[:, :, c]))
    return out


def _unmember(v, counts):
    return v[0] if counts is None else v


def rank_rhat(chain, counts=None):
    """{'bulk', 'folded', 'rhat'}, each (ncols,) or (k, ncols) with ``counts``: split R-hat of the rank-normalised pool, of
    the rank-normalised |x - median(pool)|, and their maximum (NaN when either is)."""
    def parts(pool):
        if _bad(pool):
            return np.nan, np.nan
        with np.errstate(invalid='ignore'):
            return _rhat_of(rank_normalize(pool)), _rhat_of(rank_normalize(np.abs(pool - np.median(pool))))
    v = _per_column(chain, counts, parts, (2,))
    with np.errstate(invalid='ignore'):
        out = {'bulk': v[..., 0], 'folded': v[..., 1], 'rhat': np.maximum(v[..., 0], v[..., 1])}
    return {name: _unmember(a, counts) for name, a in out.items()}


def _ess_indicator(pool, thr):
    return ess_of((pool <= thr).astype(np.float64))


def _ess_kind(pool, kind):
    if _bad(pool):
        return np.nan
    if kind == 'bulk':
        return ess_of(rank_normalize(pool))
    if kind == 'mean':
        return ess_of(pool)
    q05, q95 = np.quantile(pool, [0.05, 0.95])
    with np.errstate(invalid='ignore'):
        return np.minimum(_ess_indicator(pool, q05), _ess_indicator(pool, q95))


def ess(chain, kind='bulk', counts=None):
    """Effective sample size per column, (ncols,) or (k, ncols): 'bulk' of the rank-normalised split pool, 'tail' the
    smaller of the 5 % and 95 % quantiles' indicator ESS, 'mean' of the split pool itself."""
    if kind not in ('bulk', 'tail', 'mean'):
        raise ValueError("ess: kind must be 'bulk', 'tail' or 'mean'")
    return _unmember(_per_column(chain, counts, lambda pool: _ess_kind(pool, kind)), counts)


def ess_quantile(chain, q, counts=None):
    """ESS of the indicator I[x <= Q_q] of the split pool's quantile q (a scalar in (0, 1)), per column."""
    q = float(q)
    if not 0.0 < q < 1.0:
        raise ValueError('ess_quantile: q must lie in (0, 1)')
    fn = lambda pool: np.nan if _bad(pool) else _ess_indicator(pool, np.quantile(pool, q))
    return _unmember(_per_column(chain, counts, fn), counts)


MCSE_PROBS = (0.1586553, 0.8413447)


def mcse_quantile_of(sorted_at, S, ess_q, p):
    """(th2 - th1) / 2: sorted_at(i) is the element of zero-based rank i of the pool of S values; (a, b) the Beta(ess p + 1,
    ess (1 - p) + 1) quantiles at MCSE_PROBS.  -> (value, (rank of th1, rank of th2))."""
    from scipy.special import betaincinv
    a, b = betaincinv(ess_q * p + 1.0, ess_q * (1.0 - p) + 1.0, np.array(MCSE_PROBS))
    i1, i2 = max(int(np.floor(a * S)), 0), min(int(np.ceil(b * S)), S - 1)
    return (sorted_at(i2) - sorted_at(i1)) / 2.0, (i1, i2)


def mcse(chain, q=(0.16, 0.5, 0.84), counts=None):
    """{'mean' (ncols,), 'quantiles' (ncols, len(q))} (a leading axis k with ``counts``): the Monte-Carlo standard errors of
    the split pool's mean, std(pool, ddof=1) / sqrt(ess_mean), and of its quantiles q."""
    q = [float(p) for p in np.atleast_1d(q)]
    if any(not 0.0 < p < 1.0 for p in q):
        raise ValueError('mcse: every q must lie in (0, 1)')

    def one(pool):
        if _bad(pool):
            return np.full(1 + len(q), np.nan)
        S = pool.size
        srt = np.sort(pool, axis=None)
        out = [np.std(pool, ddof=1) / np.sqrt(ess_of(pool))]
        for p in q:
            e = _ess_indicator(pool, np.quantile(pool, p))
            out.append(mcse_quantile_of(lambda i: srt[i], S, e, p)[0] if np.isfinite(e) else np.nan)
        return np.array(out)
    v = _per_column(chain, counts, one, (1 + len(q),))
    return {'mean': _unmember(v[..., 0], counts), 'quantiles': _unmember(v[..., 1:], counts)}
