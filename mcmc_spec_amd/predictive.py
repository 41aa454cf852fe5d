"""Posterior predictive checks on the GPU (include/msx.h, msx_predictive_batch / msx_series_predictive; DESIGN.md section
22): does the model reproduce the data, and which data carry chi^2?  The reference answers with its ``all_spec`` figure
(mft6.py:2361-2438) for a handful of samples; here a whole chain is streamed through the model once more and reduced per
data pixel on the device --

  * the posterior band of the median-scaled composite and of each star: mean, variance, min, max, exact quantiles;
  * the residual the likelihood compares: the continuum-normalised data, z = (model - data_n) / sigma and z^2, averaged;
  * per sample the likelihood's three terms and their weighted sum (mft6.py:1179-1191).

``check`` takes host samples, ``check_series`` a chain held on the device (a ``_lib.Series``).  Only samples that can be
evaluated enter the reductions; every reduced number depends on the ordered list of those samples alone."""
import numpy as np

from . import _lib

TERM_NAMES = ('chi_spec', 'chi_contrast', 'chi_phot', 'chi_total')
DEFAULT_Q = (0.16, 0.5, 0.84)


def _check_q(q):
    from .summary import _check_q as chk
    return chk(q)


def _scratch_bytes(scratch_mb):
    if scratch_mb is None:
        return 0
    b = int(round(float(scratch_mb) * (1 << 20)))
    if b < 1:
        raise ValueError('scratch_mb must be positive (None: the default, 256 MiB)')
    return b


def min_scratch_bytes(engine, n):
    """The smallest ``scratch_bytes`` the calls accept for ``n`` samples of ``engine``'s problem: one model row, or one
    pixel's values of the n samples in each of the 1 + nspec + 3 rows (include/msx.h)."""
    return 8 * max(int(engine.tables.prob.npix), (engine.nspec + 4) * int(n))


def _result(band, quant, resid, count):
    return {'count': int(count), 'mean': band[0], 'var': band[1], 'min': band[2], 'max': band[3], 'quantiles': quant,
            'data_norm': resid[0], 'z_mean': resid[1], 'z2_mean': resid[2]}


def check(engine, theta, q=DEFAULT_Q, scratch_mb=None, scratch_bytes=None):
    """The check over the samples ``theta`` (n, ndim) on ``engine`` (staged problem and products): a dict with ``count``
    (the samples that could be evaluated), ``mean``, ``var`` (ddof = 1), ``min``, ``max`` (1 + nspec, npix) -- row 0 the
    median-scaled composite, rows 1.. each star, in pixel order --, ``quantiles`` (len(q), 1 + nspec, npix), NumPy's
    default quantiles, ``data_norm``, ``z_mean``, ``z2_mean`` (npix,), ``terms`` (n, 4) in the order of ``TERM_NAMES`` (NaN
    where ``status`` is not 0) and ``status`` (n,).  ``scratch_mb``: the bound on the temporary device memory (None: 256
    MiB); the numbers do not depend on it."""
    q = _check_q(q)
    theta = np.atleast_2d(_lib.as_f64(theta))
    sb = _scratch_bytes(scratch_mb) if scratch_bytes is None else int(scratch_bytes)
    band, quant, resid, terms, status, count = engine.ctx.predictive_batch(theta, engine.nspec, int(engine.tables.prob.npix), q, sb)
    out = _result(band, quant, resid, count)
    out['terms'] = terms
    out['status'] = status
    return out


def check_series(series, n, engines, q=DEFAULT_Q, discard=0, thin=1, terms=False, scratch_mb=None):
    """``check`` over rows[0:n][discard::thin] of the device chain ``series``, member m's walkers flattened in (row, walker)
    order and evaluated with ``engines[m]``: a list of one dict per member (``check``'s, with ``worst_status`` in place of
    ``terms`` and ``status``).  ``terms=True``: also a ``_lib.Series`` of ndim 4 with the same members that holds the four
    terms of EVERY row 0 .. n - 1 -- ``summary.summary_of``, ``Series.acf`` and ``Series.moments`` work on it as on any
    chain; the caller closes it."""
    q = _check_q(q)
    engines = [engines] if not isinstance(engines, (list, tuple)) else list(engines)
    n = int(n)
    dst = _lib.Series(engines[0].ctx, series.nw, 4, series.counts, cap_hint=max(n, 1)) if terms else None
    try:
        parts, count, worst = series.predictive([e.ctx for e in engines], [int(e.tables.prob.npix) for e in engines], n, discard, thin,
                                                q, _scratch_bytes(scratch_mb), dst)
    except Exception:
        if dst is not None:
            dst.close()
        raise
    out = []
    for m, (band, quant, resid) in enumerate(parts):
        d = _result(band, quant, resid, count[m])
        d['worst_status'] = int(worst[m])
        out.append(d)
    return (out, dst) if terms else out


def report(res, wl=None):
    """What the examples print of a ``check`` / ``get_predictive`` dict: the share of sum(z2_mean) carried by the worst 1 %
    of the pixels, and the largest |z_mean| with its pixel (and wavelength, given ``wl``)."""
    z2 = np.asarray(res['z2_mean'])
    nworst = max(1, int(np.ceil(0.01 * z2.size)))
    share = float(np.sort(z2)[-nworst:].sum() / z2.sum())
    p = int(np.argmax(np.abs(res['z_mean'])))
    return {'worst_share': share, 'worst_pixels': nworst, 'max_abs_z': float(abs(res['z_mean'][p])), 'pixel': p,
            'wavelength': None if wl is None else float(np.asarray(wl)[p])}


def print_report(res, wl=None, label=''):
    """The examples' three lines for a ``check`` dict: the posterior means of the three terms, the share of sum(z2_mean)
    carried by the worst 1 % of the pixels, and the largest |z_mean| with its wavelength."""
    r = report(res, wl)
    ok = np.asarray(res['status']) == 0
    means = np.mean(np.asarray(res['terms'])[ok], axis=0) if ok.any() else np.full(4, np.nan)
    print('{}predictive check over {} samples: <chi_spec> {:.4g} (per pixel)  <chi_contrast> {:.4g}  <chi_phot> {:.4g}  <chi_total> {:.4g}'.format(
        label, res['count'], *means))
    print('{}  the worst {} pixels (1 %) carry {:.1f} % of sum <z^2>'.format(label, r['worst_pixels'], 100.0 * r['worst_share']))
    where = 'pixel {}'.format(r['pixel']) if r['wavelength'] is None else '{:.5g} um'.format(r['wavelength'])
    print('{}  largest |<z>| = {:.3g} sigma at {}'.format(label, r['max_abs_z'], where))

