"""The rank-normalised diagnostics of DESIGN.md section 26 written out a second time, for tests: loops, math.fsum, SciPy's
rankdata / ndtri / betaincinv -- nothing shared with mcmc_spec_amd.diagnostics but the paper (Vehtari et al. 2021)."""
import math

import numpy as np
from scipy.special import betaincinv, ndtri
from scipy.stats import rankdata


def pool_of(x):
    """(h, J) of one member's column x (n', W): half-chain j = 2 w + half."""
    n, W = x.shape
    h = n // 2
    out = np.empty((h, 2 * W))
    for w in range(W):
        out[:, 2 * w] = x[:h, w]
        out[:, 2 * w + 1] = x[n - h:, w]
    return out


def zscores(pool):
    S = pool.size
    r = rankdata(pool.ravel(), method='average').reshape(pool.shape)
    return ndtri((r - 0.375) / (S + 0.25))


def rhat(y):
    h, J = y.shape
    m = [math.fsum(y[:, j]) / h for j in range(J)]
    s2 = [math.fsum((y[:, j] - m[j]) ** 2) / (h - 1) for j in range(J)]
    within = math.fsum(s2) / J
    mbar = math.fsum(m) / J
    between = math.fsum((v - mbar) ** 2 for v in m) / (J - 1)
    return math.sqrt(((h - 1) / h * within + between) / within)


def geyer(y):
    """(ESS, max_t, the sum of the pair at which the positive sequence ended, the pairs the monotone sequence levelled) of the
    chains y (h, J)."""
    h, J = y.shape
    S = h * J
    m = [math.fsum(y[:, j]) / h for j in range(J)]
    d = y - np.array(m)

    def A(t):
        return math.fsum(math.fsum(d[:h - t, j] * d[t:, j]) / h for j in range(J)) / J
    mean_var = A(0) * h / (h - 1)
    mbar = math.fsum(m) / J
    var_plus = mean_var * (h - 1) / h + math.fsum((v - mbar) ** 2 for v in m) / (J - 1)

    def rho(t):
        return 1.0 - (mean_var - A(t)) / var_plus
    seq = {0: 1.0, 1: rho(1)}
    even, odd, t = 1.0, seq[1], 1
    while t < h - 3 and even + odd > 0.0:
        even, odd = rho(t + 1), rho(t + 2)
        if even + odd >= 0.0:
            seq[t + 1], seq[t + 2] = even, odd
        t += 2
    max_t = t - 2
    if even > 0.0:
        seq[max_t + 1] = even
    levelled = 0
    for u in range(1, max_t - 1, 2):
        if seq[u + 1] + seq[u + 2] > seq[u - 1] + seq[u]:
            seq[u + 1] = seq[u + 2] = (seq[u - 1] + seq[u]) / 2.0
            levelled += 1
    tau = -1.0 + 2.0 * math.fsum(seq.get(i, 0.0) for i in range(max_t + 1)) + seq.get(max_t + 1, 0.0)
    return S / max(tau, 1.0 / math.log10(S)), max_t, even + odd, levelled


def everything(x, q=(0.16, 0.5, 0.84)):
    """One member's column x (n', W) -> the dict of every statistic."""
    pool = pool_of(x)
    S = pool.size
    srt = np.sort(pool.ravel())
    ind = lambda thr: (pool <= thr).astype(float)
    out = {'bulk': rhat(zscores(pool)), 'folded': rhat(zscores(np.abs(pool - np.median(pool))))}
    out['rhat'] = max(out['bulk'], out['folded'])
    out['ess_bulk'] = geyer(zscores(pool))[0]
    out['ess_tail'] = min(geyer(ind(np.quantile(pool, 0.05)))[0], geyer(ind(np.quantile(pool, 0.95)))[0])
    out['ess_mean'] = geyer(pool)[0]
    out['mcse_mean'] = np.std(pool, ddof=1) / math.sqrt(out['ess_mean'])
    out['ess_quantile'], out['mcse_quantile'] = [], []
    for p in q:
        e = geyer(ind(np.quantile(pool, p)))[0]
        a, b = betaincinv(e * p + 1.0, e * (1.0 - p) + 1.0, [0.1586553, 0.8413447])
        th1, th2 = srt[max(int(math.floor(a * S)), 0)], srt[min(int(math.ceil(b * S)), S - 1)]
        out['ess_quantile'].append(e)
        out['mcse_quantile'].append((th2 - th1) / 2.0)
    return out


def close(a, b, rtol):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    return a.shape == b.shape and bool(np.all(np.abs(a - b) <= rtol * np.abs(b)))


def ar1(n, W, rho, seed):
    rng = np.random.default_rng(seed)
    e = rng.standard_normal((n, W))
    x = np.empty((n, W))
    x[0] = e[0] / math.sqrt(1.0 - rho * rho)
    for i in range(1, n):
        x[i] = rho * x[i - 1] + e[i]
    return x


def cut_margin(y):
    """The smallest |rho(t + 1) + rho(t + 2)| over the pairs Geyer's positive sequence looks at on the chains y (h, J), by the
    definition's own autocovariance: a cut decided by roundoff shows as a margin near zero.  inf when no pair is looked at or
    the pool has no ESS."""
    from mcmc_spec_amd import diagnostics
    h, J = y.shape
    if not np.all(np.isfinite(y)) or np.all(y == y.flat[0]):
        return np.inf
    A, mean_var, between = diagnostics.chain_acov(y)
    var_plus = mean_var * (h - 1) / h + between
    with np.errstate(invalid='ignore', divide='ignore'):
        rho = 1.0 - (mean_var - A) / var_plus
    even, odd, t, margin = 1.0, rho[1], 1, np.inf
    while t < h - 3 and even + odd > 0.0:
        even, odd = rho[t + 1], rho[t + 2]
        margin = min(margin, abs(even + odd))
        t += 2
    return margin


def margins(x, counts, q=(0.16, 0.5, 0.84)):
    """The smallest cut_margin over every pool whose ESS the statistics of the selection x (n', W, ncols) need."""
    from mcmc_spec_amd import diagnostics
    worst = np.inf
    for xm in diagnostics._members(x, counts):
        for c in range(xm.shape[2]):
            pool = diagnostics.split_pool(xm[:, :, c])
            if not np.all(np.isfinite(pool)) or np.all(pool == pool.flat[0]):
                continue
            ys = [diagnostics.rank_normalize(pool), pool] + [(pool <= np.quantile(pool, p)).astype(float) for p in (0.05, 0.95) + tuple(q)]
            worst = min([worst] + [cut_margin(y) for y in ys])
    return worst
