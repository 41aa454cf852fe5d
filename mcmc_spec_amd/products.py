"""Derived posteriors on the GPU (include/msx.h, msx_stage_products / msx_products_batch / msx_series_derive; DESIGN.md
section 15): what the reference's ``plot_results`` computes from chain samples after the run --

  * the Kepler-band magnitude of each star and their contrast, ``kep_contrast.txt`` (mft6.py:2486-2539);
  * the planet-radius correction factors ``pri_corr.txt`` / ``sec_corr.txt`` (:2544-2593);
  * the Gaia G magnitudes of the components, ``gaia_pri.txt`` / ``gaia_sec.txt`` (:2540-2541);
  * mass and luminosity posteriors from the isochrone (:2679-2721)

-- by running every sample back through ``make_composite(..., plot=True)`` (:786-828).  Here a sample is one GPU thread:
the band integrals are per-node tables built at staging, so a derived value is a recipe and a few look-ups.  ``stage``
registers the Kepler and Gaia curves on an engine, ``evaluate`` maps samples to columns, ``derive`` maps a chain held on
the device (a ``_lib.Series``) to a series of derived columns that ``mcmc_spec_amd.summary`` then summarises."""
import os

import numpy as np

from . import _lib
from . import staging

# names of derived columns: `name` or `name:index`
_SIMPLE = {
    'kep_pri': lambda p: _lib.pcol_bandmag(p['kepler'], 0), 'kep_sec': lambda p: _lib.pcol_bandmag(p['kepler'], 1),
    'kep_ter': lambda p: _lib.pcol_bandmag(p['kepler'], 2), 'kep_sum': lambda p: _lib.pcol_bandmag_sum(p['kepler']),
    'kep_contrast': lambda p: _lib.pcol_dmag(p['kepler'], 1), 'kep_contrast_ter': lambda p: _lib.pcol_dmag(p['kepler'], 2),
    'pri_corr': lambda p: _lib.pcol_pri_corr(p['kepler']), 'sec_corr': lambda p: _lib.pcol_sec_corr(p['kepler']),
    'gaia_pri': lambda p: _lib.pcol_bandmag(p['gaia'], 0), 'gaia_sec': lambda p: _lib.pcol_bandmag(p['gaia'], 1),
    'gaia_ter': lambda p: _lib.pcol_bandmag(p['gaia'], 2), 'gaia_sum': lambda p: _lib.pcol_bandmag_sum(p['gaia']),
    'gaia_contrast': lambda p: _lib.pcol_dmag(p['gaia'], 1),
}
_INDEXED = {'contrast': _lib.pcol_contrast, 'phot': _lib.pcol_phot, 'logg': _lib.pcol_logg, 'mass': _lib.pcol_mass,
            'lum': _lib.pcol_lum, 'coord': int}
# the reference's workload: what plot_results derives for every one of its 2,000 samples of a binary
REFERENCE_COLUMNS = ('kep_contrast', 'pri_corr', 'sec_corr', 'gaia_pri', 'gaia_sec', 'mass:0', 'mass:1', 'lum:0', 'lum:1')


def columns(names, bands=None):
    """Names -> codes (include/msx.h, MSX_PCOL_*).  A name is one of ``kep_pri, kep_sec, kep_ter, kep_sum, kep_contrast
    (= kep_sec - kep_pri, mft6.py:2505), kep_contrast_ter, pri_corr, sec_corr (:2544-2545), gaia_pri, gaia_sec, gaia_ter,
    gaia_sum, gaia_contrast``, or indexed: ``contrast:f`` / ``phot:p`` (the staged problem's filter f / band p),
    ``logg:s`` / ``mass:s`` / ``lum:s`` (star s), ``coord:c`` (the sample's own coordinate c).  An integer is taken as a
    code.  ``bands``: the positions of the product bands, ``{'kepler': 0, 'gaia': 1}`` as ``stage`` lays them out."""
    pos = {'kepler': 0, 'gaia': 1}
    pos.update(bands or {})
    out = []
    for nm in ([names] if isinstance(names, (str, int, np.integer)) else list(names)):
        if isinstance(nm, (int, np.integer)):
            out.append(int(nm))
            continue
        key, _, idx = str(nm).partition(':')
        if key in _SIMPLE and not idx:
            out.append(_SIMPLE[key](pos))
        elif key in _INDEXED and idx.isdigit():
            out.append(_INDEXED[key](int(idx)))
        else:
            raise ValueError('unknown derived column {!r}'.format(nm))
    return out


def names_of(codes):
    """The inverse of ``columns`` for the default band positions (codes that no name produces come back as integers)."""
    back = {}
    for nm in _SIMPLE:
        back.setdefault(columns(nm)[0], nm)
    out = []
    for c in codes:
        kind, _, idx = _lib.pcol_decode(c)
        by_kind = {6: 'contrast', 7: 'phot', 8: 'logg', 9: 'mass', 10: 'lum', 0: 'coord'}
        out.append(back.get(int(c), '{}:{}'.format(by_kind[kind], idx) if kind in by_kind else int(c)))
    return out


def stage(engine, kepler, gaia=None, matrix=None, kepler_kind=None, log_columns=False):
    """Stage the product bands beside ``engine``'s staged problem (msx_stage_products): ``kepler = (wl [A], tm)`` as
    ``get_transmission('kepler', res)`` gives it -- band 0, the binary's trapezoid integral (mft6.py:792-799) or, for a
    triple, the plain sum (:820-822) -- and ``gaia``, a ``bands.Band`` with an optional ``zero_mag`` attribute -- band 1,
    ``lib['Gaia_G']`` (:811-814).  ``matrix``: the isochrone table mass and luminosity come from (its first 200 rows of
    age 9.0, :2604-2605).  To be called again whenever the problem is staged again."""
    st = engine.tables
    if st is None:
        raise RuntimeError('stage the problem first (Engine.stage_problem)')
    if matrix is None:
        raise ValueError('products.stage needs the isochrone matrix (mass and luminosity columns)')
    kind = kepler_kind or ('trapz' if engine.nspec == 2 else 'sum')
    pt = staging.build_products(engine.grid['wl'], st.r, st.tmi, st.tma, engine._tm[0], engine._tm[1], matrix, kepler, gaia,
                                kepler_kind=kind, log_columns=log_columns)
    engine.ctx.stage_products(pt.prod)
    engine.products = pt
    return pt


def _codes(cols):
    return columns(cols) if not isinstance(cols, np.ndarray) else [int(c) for c in cols]


def evaluate(engine, theta, cols, with_status=False):
    """The derived columns ``cols`` (names or codes) of the samples ``theta`` (n, ndim) or (ndim,): (n, ncols), NaN where a
    sample cannot be evaluated (msx_products_batch); with ``with_status`` also the samples' MSX_W_* codes."""
    theta = np.asarray(theta, dtype=float)
    th = np.atleast_2d(theta)
    out, status = engine.ctx.products_batch(th, _codes(cols))
    out = out[0] if theta.ndim == 1 else out
    return (out, status) if with_status else out


def derive(series, engines, cols, n=None, dst=None):
    """Rows 0 .. n - 1 of the device chain ``series`` (a ``_lib.Series`` of ndim = 2 nspec + 2) mapped to the derived
    columns ``cols``: a ``_lib.Series`` of ndim = len(cols) with the same members, member m evaluated with
    ``engines[m]`` (msx_series_derive).  ``summary.summary_of`` / ``marginals`` / ``corner_counts`` and ``Series.acf``
    work on it as on any chain.  ``dst``: a series to write into (rows 0 .. n - 1 are overwritten)."""
    engines = [engines] if not isinstance(engines, (list, tuple)) else list(engines)
    codes = _codes(cols)
    n = series.rows if n is None else int(n)
    if dst is None:
        dst = _lib.Series(engines[0].ctx, series.nw, len(codes), series.counts, cap_hint=n)
    dst.worst_status = series.derive([e.ctx for e in engines], codes, dst, 0, n)
    return dst


def spectra(engine, theta, median_scale=True, with_status=False):
    """The spectra of the samples ``theta`` (n, ndim) or (ndim,) on the staged problem's data pixels, in pixel order:
    ``(spec (n, 1 + nspec, npix), scale (n,))`` -- rows 1.. each star's spectrum, reddened by the sample's A_V on the model
    grid and resampled (mft6.py:2394-2402), row 0 their sum, multiplied by ``median(data) / median(row 0)`` (:2409; the
    factor comes back as ``scale``) when ``median_scale`` (msx_products_spectra).  NaN where a sample cannot be evaluated."""
    theta = np.asarray(theta, dtype=float)
    th = np.atleast_2d(theta)
    npix = int(engine.tables.prob.npix)
    out, scale, status = engine.ctx.products_spectra(th, engine.nspec, npix, median_scale)
    if theta.ndim == 1:
        out, scale = out[0], scale[0]
    return (out, scale, status) if with_status else (out, scale)


# the zero points make_composite(plot=True) divides a triple's Kepler sums by (mft6.py:758-761): [r, i, z, J, H, Ks] in Jy
# (2MASS: Cohen et al. 2003; SDSS: the SVO filter profile service), central wavelengths and widths in Angstrom
TRIPLE_ZP_JY = [3112.91, 2502.62, 1820.98, 1594, 1024, 666.7]
TRIPLE_CW = [6246.98, 7718.28, 10829.83, 1.235e4, 1.662e4, 2.159e4]
TRIPLE_BP_WIDTH = [1253.71, 1478.93, 4306.72, 1620, 2509, 2618]
TRIPLE_ZP = [TRIPLE_ZP_JY[n] * TRIPLE_BP_WIDTH[n] / (3.336e4 * TRIPLE_CW[n] ** 2) for n in range(6)]


def _summary_of_values(ctx, values, q):
    """get_summary's dict (one member) of host values (N, ncols), through a temporary one-walker series."""
    from . import summary
    with summary.uploaded(values[:, None, :], ctx) as (series, n):
        out = summary.summary_of(series, n, q)
    return {name: v[0] for name, v in out.items()}


def summarize_chain(series, n, engines, cols, q=(0.16, 0.5, 0.84), discard=0, thin=1):
    """``summary.summary_of`` over the derived columns of rows[0:n][discard::thin] of a device chain: derive, then one
    order-statistics call; (k, ...) arrays as summary_of returns them."""
    from . import summary
    dst = derive(series, engines, cols, n)
    try:
        return summary.summary_of(dst, n, q, None, discard, thin)
    finally:
        dst.close()


def reference_files(dirname, values, ratio=None):
    """Write the files plot_results leaves in its run directory, with ``np.savetxt`` as it does (mft6.py:2539-2541,
    :2576, :2593, :2721).  ``values``: {name: 1-D array} with any of ``kep_contrast, gaia_sec, gaia_pri, pri_corr,
    sec_corr, primary_mass_posterior, secondary_mass_posterior, primary_lum_posterior, secondary_lum_posterior``;
    ``pri_corr`` / ``sec_corr`` are computed from ``kep_contrast`` (and ``ratio``, the samples' R2 / R1) by the
    reference's statements (:2544-2545) when they are not given.  Returns the paths written."""
    vals = {k: np.asarray(v, dtype=float) for k, v in values.items()}
    if 'kep_contrast' in vals:
        kc = vals['kep_contrast']
        vals.setdefault('pri_corr', np.sqrt(1 + 10 ** (-0.4 * kc)))  # mft6.py:2544
        if ratio is not None:
            vals.setdefault('sec_corr', np.asarray(ratio, dtype=float) * np.sqrt(1 + 10 ** (0.4 * kc)))  # mft6.py:2545
    known = ['kep_contrast', 'gaia_sec', 'gaia_pri', 'pri_corr', 'sec_corr', 'primary_mass_posterior',
             'secondary_mass_posterior', 'primary_lum_posterior', 'secondary_lum_posterior']
    unknown = sorted(set(vals) - set(known))
    if unknown:
        raise ValueError('reference_files: unknown entries ' + ', '.join(unknown))
    os.makedirs(dirname, exist_ok=True)
    paths = []
    for name in known:
        if name in vals:
            path = os.path.join(dirname, name + '.txt')
            np.savetxt(path, np.array(vals[name]))
            paths.append(path)
    return paths
