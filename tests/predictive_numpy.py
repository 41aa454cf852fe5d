"""The NumPy twin of the posterior predictive check (include/msx.h, msx_predictive_batch): the
reductions of a given array of spectra with np.mean / np.var(ddof=1) / np.min / np.max / np.quantile, and data_n, z and the
likelihood's terms from the oracle's norm_spec / chisq -- the arithmetic of
tests/test_gpu_products.py::test_spectra_close_the_loop_with_the_hot_path."""
import numpy as np

from oracle import mft6_oracle as orc

TERM_NAMES = ('chi_spec', 'chi_contrast', 'chi_phot', 'chi_total')


def reduce(S, q=(0.16, 0.5, 0.84), status=None):
    """The band of S (n, rows, npix) over the samples whose status is 0 (None: all): {'count', 'mean', 'var', 'min', 'max'
    (rows, npix), 'quantiles' (len(q), rows, npix)}; count 0 gives NaN everywhere, count 1 a NaN variance."""
    S = np.asarray(S, dtype=float)
    if status is not None:
        S = S[np.asarray(status) == 0]
    n = S.shape[0]
    shape = S.shape[1:]
    if n == 0:
        nan = np.full(shape, np.nan)
        return {'count': 0, 'mean': nan, 'var': nan.copy(), 'min': nan.copy(), 'max': nan.copy(),
                'quantiles': np.full((len(q),) + shape, np.nan)}
    var = np.var(S, axis=0, ddof=1) if n > 1 else np.full(shape, np.nan)
    return {'count': n, 'mean': np.mean(S, axis=0), 'var': var, 'min': np.min(S, axis=0), 'max': np.max(S, axis=0),
            'quantiles': np.quantile(S, q, axis=0)}


def two_pass_var(S):
    """The variance the header promises: the float64 mean first, then sum (x - mean)^2 / (n - 1)."""
    S = np.asarray(S, dtype=float)
    mean = np.mean(S, axis=0)
    return np.sum((S - mean) ** 2, axis=0) / (S.shape[0] - 1)


def residuals(c, model):
    """(data_n, z) (n, npix) of the scaled composites ``model`` (n, npix) of case c: norm_spec (mft6.py:193-196, :1174) and
    z = (model - data_n) / err, so that chisq (:115-120) is z^2."""
    wl, spec, err = np.asarray(c.data[0]), np.asarray(c.data[1]), np.asarray(c.err)
    data_n = np.array([orc.norm_spec(wl, m, spec) for m in np.atleast_2d(model)])
    return data_n, (np.atleast_2d(model) - data_n) / err


def terms(c, theta, model, contrast, phot):
    """(n, 4) chi_spec, chi_contrast, chi_phot, chi_total (mft6.py:1179-1191) from the scaled composites ``model`` (n, npix)
    and the unreddened band terms ``contrast`` (n, nc), ``phot`` (n, nph) of the samples ``theta``."""
    nc, nph = len(c.fr[2]), len(c.fr[5])
    phot_cwl = np.array([float(x) for x in c.ptm[3]][:nph])
    out = []
    for i, p in enumerate(np.atleast_2d(theta)):
        a_v = p[c.nspec]
        spec_n = orc.norm_spec(np.asarray(c.data[0]), model[i], np.asarray(c.data[1]))
        ic = orc.chisq(model[i], spec_n, c.err)
        iic = np.sum(ic) / len(ic)
        ph = phot[i]
        if a_v > 0 and nph:
            ph = -2.5 * np.log10(orc.extinct(phot_cwl, 10 ** (-0.4 * ph), a_v))  # mft6.py:1163
        chi_c, chi_p = np.sum(orc.chisq(contrast[i], c.fr[0], c.fr[1])), np.sum(orc.chisq(ph, c.fr[3], c.fr[4]))
        out.append([iic, chi_c, chi_p, np.sum((iic * (nc + nph), chi_c, chi_p))])
    return np.array(out, dtype=float).reshape(-1, 4)


def check(c, theta, S, contrast, phot, q=(0.16, 0.5, 0.84), status=None):
    """mcmc_spec_amd.predictive.check's dict from the samples' spectra S (n, 1 + nspec, npix) (row 0 median-scaled)."""
    S = np.asarray(S, dtype=float)
    n = S.shape[0]
    status = np.zeros(n, dtype=np.int32) if status is None else np.asarray(status, dtype=np.int32)
    ok = status == 0
    out = reduce(S, q, status)
    npix = S.shape[2]
    t = np.full((n, 4), np.nan)
    if ok.any():
        t[ok] = terms(c, np.atleast_2d(theta)[ok], S[ok, 0], np.atleast_2d(contrast)[ok], np.atleast_2d(phot)[ok])
        data_n, z = residuals(c, S[ok, 0])
        out.update(data_norm=np.mean(data_n, axis=0), z_mean=np.mean(z, axis=0), z2_mean=np.mean(z ** 2, axis=0))
    else:
        out.update(data_norm=np.full(npix, np.nan), z_mean=np.full(npix, np.nan), z2_mean=np.full(npix, np.nan))
    out.update(terms=t, status=status)
    return out
