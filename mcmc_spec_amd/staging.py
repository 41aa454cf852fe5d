"""Host-side staging: turn the reference's Python arguments into the dense tables the HIP library
consumes (``struct msx_problem``, include/msx.h).

Nothing here touches model fluxes: the grid goes to HBM once (``stage_specs``) and every
flux-dependent table (pixel pair table, per-node band integrals, CCM89 curve, broadened nodes) is
produced on the device by ``libmsx.so``.  What *is* computed here are the walker-independent index
and weight tables, with the same NumPy/SciPy expressions the reference uses so that masks and
``searchsorted`` decisions are bit-identical (SURVEY.md §7 "bit-level staging semantics").
"""
from __future__ import annotations

import ctypes as C

import numpy as np
from numpy.polynomial import polyutils as pu
from scipy.interpolate import interp1d

from . import _lib
from .bands import BAND_NAMES_3, BAND_NAMES_6, _trapz_weights


def parse_specs(specs):
    """``specs`` dict (mft6.py:363,383) -> (teff_nodes, logg_nodes, wl, flux[nt][ng][nwl], present).

    Node values come from the dict keys (the reference re-lists the model directory instead,
    mft6.py:423-436).  Absent (T, g) combinations are marked not-present: touching
    one raises KeyError at evaluation time like the reference (mft6.py:489-500)."""
    ts, gs = set(), set()
    for k in specs:
        if k == 'wl':
            continue
        a, b = k.split(', ')
        ts.add(int(a))
        gs.add(float(b))
    teff = sorted(ts)
    logg = sorted(gs)
    wl = np.asarray(specs['wl'], dtype=np.float64)
    flux = np.zeros((len(teff), len(logg), len(wl)))
    present = np.zeros((len(teff), len(logg)), dtype=np.uint8)
    for it, t in enumerate(teff):
        for ig, g in enumerate(logg):
            v = specs.get('{}, {}'.format(t, g))
            if v is not None:
                flux[it, ig] = v
                present[it, ig] = 1
    return np.array(teff, dtype=float), np.array(logg, dtype=float), wl, flux, present


def parse_component_specs(specs_seq):
    """A tuple of ``nspec`` ``specs`` dicts, one per star (an extension of the reference's ``specs`` argument) ->
    (teff_nodes, logg_nodes, wl, flux[ncomp][nt][ng][nwl], present).  The dicts must share their keys and ``wl``
    exactly: ValueError otherwise."""
    specs_seq = list(specs_seq)
    if not 1 <= len(specs_seq) <= 3:
        raise ValueError('specs: one dict per star, 1 to 3 of them ({} given)'.format(len(specs_seq)))
    for s, d in enumerate(specs_seq):
        if not isinstance(d, dict):
            raise ValueError('specs[{}]: a specs dict expected, got {}'.format(s, type(d).__name__))
    keys0 = set(specs_seq[0])
    wl0 = np.asarray(specs_seq[0]['wl'], dtype=np.float64)
    for s, d in enumerate(specs_seq[1:], 1):
        if set(d) != keys0:
            raise ValueError('specs[{}] does not have the keys of specs[0]: the per-star dicts must share their nodes'.format(s))
        w = np.asarray(d['wl'], dtype=np.float64)
        if w.shape != wl0.shape or not np.array_equal(w, wl0):
            raise ValueError("specs[{}]['wl'] differs from specs[0]['wl']: the per-star dicts must share one axis".format(s))
    parts = [parse_specs(d) for d in specs_seq]
    teff, logg, wl, _, present = parts[0]
    return teff, logg, wl, np.stack([p[3] for p in parts]), present


def composite_window_um(r, tmi, tma, ctm, ptm):
    """The window make_composite passes to get_spec, in micron (mft6.py:663-673,687)."""
    wlmin, wlmax = np.inf, 0
    for w in list(ctm[0]) + list(ptm[0]):
        if min(w) < wlmin:
            wlmin = min(w)
        if max(w) > wlmax:
            wlmax = max(w)
    return [min(min(r), tmi / 1e4, wlmin / 1e4) - 1e-4, max(max(r), tma / 1e4, wlmax / 1e4) + 1e-4]


def window_slice(wl, reg_um):
    """Contiguous [j0, j0+n) selected by get_spec's crop masks (mft6.py:537-542)."""
    lim = np.array(reg_um) * 1e4
    keep = np.where((wl >= min(lim)) & (wl <= max(lim)))[0]
    if keep.size == 0:
        raise ValueError('the composite window selects no model samples')
    if keep[-1] - keep[0] + 1 != keep.size:
        raise ValueError('model wavelength grid must be sorted')
    return int(keep[0]), int(keep.size)


def resample_tables(wave, x):
    """np.interp / interp1d(kind='linear') bracket of each query (mft6.py:1169-1170).

    Returns (lo, t) with result = y[lo] + (y[lo+1]-y[lo])*t.  Raises the same ValueError scipy does
    when a query lies outside [wave[0], wave[-1]]."""
    if np.any(np.diff(wave) <= 0):
        raise ValueError('model wavelength grid must be strictly increasing')
    if np.any(x < wave[0]):
        raise ValueError("A value ({}) in x_new is below the interpolation range's minimum value ({})."
                         .format(x.min(), wave[0]))
    if np.any(x > wave[-1]):
        raise ValueError("A value ({}) in x_new is above the interpolation range's maximum value ({})."
                         .format(x.max(), wave[-1]))
    j = np.searchsorted(wave, x, side='right') - 1
    last = j >= len(wave) - 1
    j = np.where(last, len(wave) - 2, j)
    t = (x - wave[j]) / (wave[j + 1] - wave[j])
    t = np.where(last, 1.0, t)
    return j.astype(np.int64), t


def contrast_weights(wave, ran, tm):
    """Weights for one contrast filter: ``trapz(s*tran, w)`` over the in-band samples (mft6.py:719-731)."""
    ran = np.asarray(ran, dtype=float)
    inband = np.where((wave <= max(ran)) & (wave >= min(ran)))[0]
    if inband.size < 2:
        raise ValueError('a contrast filter does not overlap the model window')
    w = wave[inband]
    tran = interp1d(ran, tm)(w)
    return int(inband[0]), _trapz_weights(w) * tran


def sorted_isochrone(matrix):
    """1 Gyr rows (``matrix[:,1] == 9.0``, first 220) sorted by Teff the way interp1d sorts its x
    (stable mergesort) (mft6.py:73-76, 90-95)."""
    sel = np.where(np.asarray(matrix[:, 1]) == 9.0)[0][:220]
    x = np.asarray(matrix[sel, 4], dtype=float)
    order = np.argsort(x, kind='mergesort')
    return x[order], np.asarray(matrix[sel, 5], dtype=float)[order], np.asarray(matrix[sel, 6], dtype=float)[order]


def prior_vectors(prior, nspec, dist_fit=True):
    """The reference's ``prior`` list re-ordered to parameter order: mft6.py:1243-1254 with ``dist_fit``
    (Teff.., A_V, radii.., parallax), :1303-1312 without (Teff.., A_V and ``nspec-1`` radius entries only --
    the slices there are one element shorter and the parallax has no Gaussian term)."""
    ndim = 2 * nspec + 2
    mean, sig = np.zeros(_lib.MAX_DIM), np.ones(_lib.MAX_DIM)
    if isinstance(prior, (int, float)) and prior == 0:
        return mean, sig, 0
    prior = [float(p) for p in prior]
    if dist_fit:
        ps = prior[:nspec] + [prior[2 * nspec]] + prior[2 * nspec + 2:3 * nspec + 2] + [prior[-2]]
        ss = prior[nspec:2 * nspec] + [prior[2 * nspec + 1]] + prior[3 * nspec + 2:4 * nspec + 2] + [prior[-1]]
    else:
        ps = prior[:nspec] + [prior[2 * nspec]] + prior[2 * nspec + 2:3 * nspec + 1]
        ss = prior[nspec:2 * nspec] + [prior[2 * nspec + 1]] + prior[3 * nspec + 2:4 * nspec + 1]
    assert len(ps) <= ndim
    mean[:len(ps)] = ps
    sig[:len(ss)] = ss
    return mean, sig, 1


class StagedTables:
    """Owns the NumPy arrays referenced by a ``MsxProblem`` (keeps them alive for the ctypes call)."""

    def __init__(self):
        self.keep = []
        self.prob = _lib.MsxProblem()

    def f64(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        if a.size == 0:
            a = np.zeros(1)
        self.keep.append(a)
        return _lib.dptr(a)

    def i64(self, a):
        a = np.ascontiguousarray(a, dtype=np.int64)
        if a.size == 0:
            a = np.zeros(1, dtype=np.int64)
        self.keep.append(a)
        return _lib.iptr(a)


def build_problem(ctx, grid_wl, data, err, fr, r, ctm, ptm, tmi, tma, matrix, nspec=2, bands=None,
                  av_table=None, tmin=-np.inf, tmax=np.inf, prior=0, use_av=True, dist_fit=True, rad_prior=False,
                  spectrum=True):
    """Assemble ``struct msx_problem`` for one dataset.  Arguments follow ``logposterior``'s
    (mft6.py:1459): ``data = [wl_um, flux]``, ``fr = [cmag, cerr, cfilt, pmag, perr, pfilt]``,
    ``ctm``/``ptm`` = ``[wls, tras, n_res_el, cwl]``.  ``bands`` maps pyphot-style names to
    ``bands.Band``; ``av_table`` = (edges_pc, mu, sigma) or None."""
    st = StagedTables()
    P = st.prob
    wl_um, flux = np.asarray(data[0], dtype=float), np.asarray(data[1], dtype=float)
    err = np.asarray(err, dtype=float)
    if not (len(wl_um) == len(flux) == len(err)):
        raise ValueError('Data and model must be the same length')
    npix = len(wl_um)
    grid_wl = np.asarray(grid_wl, dtype=float)

    reg = composite_window_um(r, tmi, tma, ctm, ptm)
    j0, nwin = window_slice(grid_wl, reg)
    wave = grid_wl[j0:j0 + nwin]

    lo, t = resample_tables(wave, wl_um * 1e4)  # mft6.py:1170: intep(wl * 1e4)
    dom = pu.getdomain(wl_um)  # Polynomial.fit(wl, ...) maps its domain to [-1, 1]
    u = pu.mapdomain(wl_um, dom, np.array([-1.0, 1.0]))
    V = np.stack([np.ones_like(u), u, u * u], axis=1)
    minv = np.linalg.inv(V.T @ V)

    P.struct_size = C.sizeof(_lib.MsxProblem)
    P.nspec = int(nspec)
    P.npix = npix
    P.pix_lo = st.i64(lo + j0)
    P.pix_t = st.f64(t)
    P.pix_u = st.f64(u)
    P.pix_flux = st.f64(flux)
    P.pix_err = st.f64(err)
    P.median_flux = float(np.median(flux))
    for i in range(9):
        P.fit_minv[i] = float(minv.flat[i])

    cmag, cerr = [float(x) for x in fr[0]], [float(x) for x in fr[1]]
    nc = len(fr[2])
    pmag, perr = [float(x) for x in fr[3]], [float(x) for x in fr[4]]
    nph = len(fr[5])
    if nc > _lib.MAX_BANDS or nph > _lib.MAX_BANDS:
        raise ValueError('at most {} contrast filters and {} photometric bands'.format(_lib.MAX_BANDS, _lib.MAX_BANDS))
    i0s, lens, ws = [], [], []
    for n in range(nc):
        i0, w = contrast_weights(wave, ctm[0][n], ctm[1][n])
        i0s.append(i0 + j0)
        lens.append(len(w))
        ws.append(w)
    zero, phot_cwl = [], []
    if nph:
        if bands is None:
            raise ValueError('photometric bands requested but no band library given (see mcmc_spec_amd.bands)')
        names = BAND_NAMES_3 if nph == 3 else BAND_NAMES_6  # mft6.py:766-769
        for n in range(nph):
            b = bands[names[n]]
            i0, w = b.weights_on(wave)
            i0s.append(i0 + j0)
            lens.append(len(w))
            ws.append(w)
            zero.append(b.zero_flux)
        phot_cwl = [float(p) for p in ptm[3]][:nph]  # mft6.py:831
    P.n_contrast, P.n_phot = nc, nph
    P.band_i0 = st.i64(i0s)
    P.band_len = st.i64(lens)
    P.band_w = st.f64(np.concatenate(ws) if ws else np.zeros(0))
    P.cmag, P.cerr = st.f64(cmag), st.f64(cerr)
    P.pmag, P.perr = st.f64(pmag), st.f64(perr)
    P.phot_zero = st.f64(zero)
    P.phot_k = st.f64(ctx.ccm89_k(np.array(phot_cwl), 3.1) if nph else np.zeros(0))
    P.win_j0, P.win_n = j0, nwin

    it, ig, il = sorted_isochrone(np.asarray(matrix))
    P.niso = len(it)
    P.iso_teff, P.iso_logg, P.iso_lum = st.f64(it), st.f64(ig), st.f64(il)

    if av_table is not None:
        edges, mu, sig = av_table
        if len(edges) != len(mu) + 1 or len(mu) != len(sig):
            raise ValueError('av_table must be (edges[n+1], mu[n], sigma[n])')
        P.nav = len(mu)
        P.av_edges_pc, P.av_mu, P.av_sig = st.f64(edges), st.f64(mu), st.f64(sig)
    else:
        P.nav = 0
        P.av_edges_pc, P.av_mu, P.av_sig = st.f64([]), st.f64([]), st.f64([])
    P.tmin, P.tmax = float(tmin), float(tmax)
    mean, sig, has = prior_vectors(prior, nspec, dist_fit)
    for i in range(_lib.MAX_DIM):
        P.prior_mean[i] = mean[i]
        P.prior_sig[i] = sig[i]
    P.use_av = int(bool(use_av))
    P.dist_fit = int(bool(dist_fit))
    P.rad_prior = int(bool(rad_prior))
    P.has_prior_list = has
    P.no_spectrum = 0 if spectrum else 1  # mft6_nospec.py drops the spectrum term
    st.window = (j0, nwin)
    st.r, st.tmi, st.tma = [float(x) for x in r], float(tmi), float(tma)
    st.phot_cwl = np.array(phot_cwl)
    st.nc, st.nph = nc, nph
    return st


def isochrone_logg(teff, matrix):
    """Host-side logg(Teff) for building inputs (same table/ordering the device lookup uses)."""
    x, g, _ = sorted_isochrone(np.asarray(matrix))
    if np.any(np.asarray(teff) < x[0]) or np.any(np.asarray(teff) > x[-1]):
        raise ValueError('A value in x_new is outside the interpolation range (isochrone Teff)')
    return np.interp(teff, x, g)


def isochrone_radius(teff, matrix):
    """Host-side Stefan-Boltzmann radius [Rsun] from the isochrone luminosity (get_radius, mft6.py:66-85)."""
    x, _, lum = sorted_isochrone(np.asarray(matrix))
    if np.any(np.asarray(teff) < x[0]) or np.any(np.asarray(teff) > x[-1]):
        raise ValueError('A value in x_new is outside the interpolation range (isochrone Teff)')
    lm = np.interp(teff, x, lum)
    sigma_sb, lsun, rsun = 5.670374e-5, 3.839e33, 6.957e10
    return np.sqrt(lm * lsun / (4 * np.pi * sigma_sb * np.asarray(teff, dtype=float) ** 4)) / rsun


# ---- derived posteriors: the product bands of make_composite(plot=True) ---------------------------
def product_window_um(r, tmi, tma, ctm, ptm, kepler_wl):
    """The window make_composite passes to get_spec with ``plot=True``, in micron: the extrema of the contrast and
    photometry curves (mft6.py:663-673) with the Kepler curve's joined in (:677-682), then :687."""
    wlmin, wlmax = np.inf, 0
    for w in list(ctm[0]) + list(ptm[0]):
        if min(w) < wlmin:
            wlmin = min(w)
        if max(w) > wlmax:
            wlmax = max(w)
    if min(kepler_wl) < wlmin:
        wlmin = min(kepler_wl)
    if max(kepler_wl) > wlmax:
        wlmax = max(kepler_wl)
    return [min(min(r), tmi / 1e4, wlmin / 1e4) - 1e-4, max(max(r), tma / 1e4, wlmax / 1e4) + 1e-4]


def curve_weights(wave, ran, tm, kind):
    """(i0, w) on the window ``wave`` for one transmission curve: the samples of the reference's mask
    ``(wave >= min(ran)) & (wave <= max(ran))`` -- clipped to the window as the boolean mask clips it -- and
    ``kind='trapz'``: w with sum(w * S) = np.trapz(S[mask] * interp1d(ran, tm)(wave[mask]), wave[mask]) (mft6.py:792-799);
    ``kind='sum'``: w = the interpolated transmission, for np.sum(S[mask] * data_tm) (mft6.py:820-822)."""
    ran = np.asarray(ran, dtype=float)
    inband = np.where((wave >= min(ran)) & (wave <= max(ran)))[0]
    if inband.size < 2:
        raise ValueError('a product band does not overlap the model window')
    if inband[-1] - inband[0] + 1 != inband.size:
        raise ValueError('model wavelength grid must be sorted')
    w = wave[inband]
    tran = interp1d(ran, tm)(w)
    if kind == 'trapz':
        return int(inband[0]), _trapz_weights(w) * tran
    if kind == 'sum':
        return int(inband[0]), np.array(tran, dtype=float)
    raise ValueError("curve_weights: kind must be 'trapz' or 'sum'")


def product_isochrone(matrix, log_columns=False):
    """(teff, mass, lum) of the first 200 rows of age 9.0 (mft6.py:2604-2605, :2650, :2679), sorted by Teff the way interp1d
    sorts its x.  ``log_columns``: Teff and luminosity are stored as log10, as in the file plot_results reads (:2618);
    the default takes them as ``matrix`` holds them for get_logg / get_radius."""
    m = np.asarray(matrix)
    sel = np.where(m[:, 1] == 9.0)[0]
    t, ma, lu = np.asarray(m[sel, 4], dtype=float), np.asarray(m[sel, 3], dtype=float), np.asarray(m[sel, 6], dtype=float)
    if log_columns:
        t, lu = 10.0 ** t, 10.0 ** lu
    t, ma, lu = t[:200], ma[:200], lu[:200]
    order = np.argsort(t, kind='mergesort')
    return t[order], ma[order], lu[order]


PRODUCT_KINDS = {'trapz': _lib.PB_TRAPZ, 'sum': _lib.PB_SUM, 'mean': _lib.PB_MEAN}


def build_products(grid_wl, r, tmi, tma, ctm, ptm, matrix, kepler, gaia=None, kepler_kind='trapz', extra=(),
                   log_columns=False):
    """Assemble ``struct msx_products``.  ``kepler = (wl [A], transmission)`` as get_transmission('kepler', res) returns it:
    band 0, of ``kepler_kind`` ('trapz': the binary's integral, 'sum': the triple's).  ``gaia``: a ``bands.Band`` whose
    ``zero_mag`` attribute (default -2.5 log10(zero_flux)) is the magnitude subtracted -- band 1, of kind 'mean'.
    ``extra``: further ``(kind, curve)`` pairs, a curve being (wl, tm) or a Band.  Returns the tables (``.prod``,
    ``.window``, ``.band_names``)."""
    st = StagedTables()
    P = _lib.MsxProducts()
    grid_wl = np.asarray(grid_wl, dtype=float)
    kw, kt = np.asarray(kepler[0], dtype=float), np.asarray(kepler[1], dtype=float)
    reg = product_window_um(r, tmi, tma, ctm, ptm, kw)
    j0, nwin = window_slice(grid_wl, reg)
    wave = grid_wl[j0:j0 + nwin]
    todo = [('kepler', kepler_kind, (kw, kt))]
    if gaia is not None:
        todo.append(('gaia', 'mean', gaia))
    todo += [('extra{}'.format(i), k, cv) for i, (k, cv) in enumerate(extra)]
    if len(todo) > _lib.MAX_BANDS:
        raise ValueError('at most {} product bands'.format(_lib.MAX_BANDS))
    kinds, i0s, lens, ws, zms = [], [], [], [], []
    for name, kind, cv in todo:
        if kind == 'mean':
            i0, w = cv.weights_on(wave)
            zm = getattr(cv, 'zero_mag', None)
            zms.append(float(-2.5 * np.log10(cv.zero_flux) if zm is None else zm))
        else:
            i0, w = curve_weights(wave, cv[0], cv[1], kind)
            zms.append(0.0)
        kinds.append(PRODUCT_KINDS[kind])
        i0s.append(i0 + j0)
        lens.append(len(w))
        ws.append(w)
    P.struct_size = C.sizeof(_lib.MsxProducts)
    P.nbands = len(todo)
    ka = np.ascontiguousarray(kinds, dtype=np.int32)
    st.keep.append(ka)
    P.band_kind = ka.ctypes.data_as(C.POINTER(C.c_int32))
    P.band_i0, P.band_len = st.i64(i0s), st.i64(lens)
    P.band_w = st.f64(np.concatenate(ws))
    P.band_zero_mag = st.f64(zms)
    it, im, il = product_isochrone(matrix, log_columns)
    P.niso = len(it)
    P.iso_teff, P.iso_mass, P.iso_lum = st.f64(it), st.f64(im), st.f64(il)
    st.prod = P
    st.window = (j0, nwin)
    st.band_names = [t[0] for t in todo]
    st.band_kinds = [t[1] for t in todo]
    st.band_tables = list(zip(i0s, ws))
    st.zero_mag = np.array(zms)
    return st
