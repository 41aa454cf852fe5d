"""NumPy restatement of msx_series_acf (include/msx.h; csrc/autocorr_kernels.h) by direct sums, for the GPU tests."""
import numpy as np


def acf_direct(rows, n, discard=0, thin=1, lag0=0, nlag=None, counts=None):
    """rows (nrows, nw, ndim) -> f (k, ndim, nlag): for member m and dimension d the walker average of
    acov_k(tau) / acov_k(0), acov_k(tau) = sum_{t < n' - tau} y[t] y[t + tau], y = x - mean(x), x = rows[:n][discard::thin];
    a walker with acov_k(0) == 0 contributes ones."""
    x = np.asarray(rows, dtype=float)[:n][discard::thin]
    npr, nw, ndim = x.shape
    nlag = npr - lag0 if nlag is None else nlag
    counts = [nw] if counts is None else list(counts)
    y = (x - x.mean(axis=0)).transpose(1, 2, 0)          # (nw, ndim, n')
    a0 = np.einsum('wdt,wdt->wd', y, y)
    ratio = np.empty((nw, ndim, nlag))
    for j in range(nlag):
        tau = lag0 + j
        a = np.einsum('wdt,wdt->wd', y[:, :, :npr - tau], y[:, :, tau:])
        with np.errstate(invalid='ignore', divide='ignore'):
            ratio[:, :, j] = np.where(a0 == 0, 1.0, a / np.where(a0 == 0, 1.0, a0))
    off = np.concatenate([[0], np.cumsum(counts)])
    return np.stack([ratio[off[m]:off[m + 1]].mean(axis=0) for m in range(len(counts))])


def acf_fft_host(rows, n, discard=0, thin=1, counts=None):
    """The host method's f: the walker average of sampler._autocorr_1d, per member -> (k, ndim, n')."""
    from mcmc_spec_amd.sampler import _autocorr_1d
    x = np.asarray(rows, dtype=float)[:n][discard::thin]
    npr, nw, ndim = x.shape
    counts = [nw] if counts is None else list(counts)
    off = np.concatenate([[0], np.cumsum(counts)])
    out = np.zeros((len(counts), ndim, npr))
    for m in range(len(counts)):
        for d in range(ndim):
            for w in range(off[m], off[m + 1]):
                out[m, d] += _autocorr_1d(x[:, w, d])
            out[m, d] /= counts[m]
    return out


def ar1(nsteps, nw, ndim, rho, seed):
    rng = np.random.default_rng(seed)
    x = np.empty((nsteps, nw, ndim))
    x[0] = rng.normal(size=(nw, ndim))
    s = np.sqrt(1.0 - rho * rho)
    for t in range(1, nsteps):
        x[t] = rho * x[t - 1] + s * rng.standard_normal((nw, ndim))
    return x


def assert_not_borderline(f, c=5.0):
    """The host's window for each row of f (ndim, L) is not decided by roundoff: every index up to and including the
    window keeps |idx - c * taus[idx]| > 1e-6."""
    for fd in f:
        taus = 2.0 * np.cumsum(fd) - 1.0
        m = np.arange(len(taus)) < c * taus
        w = int(np.argmin(m)) if np.any(~m) else len(taus) - 1
        gap = np.abs(np.arange(w + 1) - c * taus[:w + 1])
        assert gap.min() > 1e-6, gap.min()
