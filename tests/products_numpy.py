"""CPU twin of the derived posteriors (mcmc_spec_amd.products): a NumPy / SciPy restatement of
what ``make_composite(..., plot=True)`` (mft6.py:786-828) returns and of what ``plot_results`` derives from it, built on
``oracle.mft6_oracle``'s public functions.  TEST INFRASTRUCTURE: pinned against the reference's own run by
``tests/golden/make_golden_products.py`` (``golden_products.npz``); the GPU tests compare the device with both."""
import numpy as np
from scipy.interpolate import interp1d

import common
from mcmc_spec_amd import synth
from oracle import mft6_oracle as orc

GOLDEN = common.GOLDEN.replace('golden_reference.npz', 'golden_products.npz')

# the triple's zero points, mft6.py:758-761: [r, i, z, J, H, Ks] (2MASS: Cohen+ 2003; SDSS: SVO filter profile service)
ZP_JY = [3112.91, 2502.62, 1820.98, 1594, 1024, 666.7]
CW = [6246.98, 7718.28, 10829.83, 1.235e4, 1.662e4, 2.159e4]
BP_WIDTH = [1253.71, 1478.93, 4306.72, 1620, 2509, 2618]
ZP = [ZP_JY[n] * BP_WIDTH[n] / (3.336e4 * CW[n] ** 2) for n in range(len(ZP_JY))]


def products_matrix():
    """The synthetic isochrone of the goldens with what the products need on top: a mass column (3) that varies, and two
    neighbouring age-9 rows (3393 K, 3410 K) whose log g is exactly the grid node 5.0, so that a Teff between them has an
    on-node log g in the reference and everywhere else."""
    m = synth.make_isochrone_matrix()
    m[:, 3] = 0.05 + 0.9 * m[:, 2] ** 1.1
    sel = np.where(m[:, 1] == 9.0)[0]
    m[sel[30:32], 5] = 5.0
    return m


def gaia_band(g, vega=None):
    """The stub ``lib['Gaia_G']`` of the goldens: photon-counting, Vega zero point from the synthetic Vega (unpinned)."""
    vw, vf = synth.synthetic_vega() if vega is None else vega
    b = orc.OracleBand(g['gaia_wl'], g['gaia_tm'], vw, vf)
    b.Vega_zero_mag = -2.5 * np.log10(b.Vega_zero_flux)
    return b


def composite_plot(c, teff, logg, rad, distance, kep_w, specs=None):
    """(wave, composite, stars) over the plot=True window: the oracle's make_composite with the Kepler curve's extrema
    joined into the window rule (mft6.py:677-682) -- an extra entry of ctm[0] that no contrast filter reads."""
    ctm = [list(c.ctm[0]) + [kep_w]] + [list(x) for x in c.ctm[1:]]
    w, comp, _, _, _, stars = orc.make_composite(teff, logg, rad, distance, c.fr[2], c.fr[5], c.r, c.specs if specs is None else specs,
                                                 ctm, c.ptm, c.tmi, c.tma, nspec=c.nspec, bandlib=c.bandlib)
    return w, comp, stars


def kepler_integrals(w, stars, ran, tm, kind):
    """The Kepler quantity of every star: np.trapz (binary, mft6.py:792-799) or np.sum (triple, :820-822; before / zp)."""
    ran = np.asarray(ran)
    mask = np.where((w >= min(ran)) & (w <= max(ran)))
    data_tm = interp1d(ran, tm)(w[mask])
    if kind == 'trapz':
        return np.array([np.trapz(np.array(s)[mask] * data_tm, w[mask]) for s in stars])
    return np.array([np.sum(np.array(s)[mask] * data_tm) for s in stars])


def sample_args(c, p, distance):
    ns = c.nspec
    tt = [float(x) for x in p[:ns]]
    if distance:
        return tt, [float(x) for x in p[ns + 1:2 * ns + 1]], float(p[2 * ns + 1])
    return tt, [float(x) for x in p[ns + 2:2 * ns + 1]], False


def evaluate(c, theta, distance, g, matrix=None):
    """The goldens' arrays for samples ``theta`` of case ``c``: {'mags', 'dkep', 'pri_corr', 'sec_corr', 'logg', 'mass',
    'lum'} ('mags': binary [kep_pri, kep_sec, gaia_pri, gaia_sec, gaia_sum]; triple [3][6], each the / zp array)."""
    matrix = products_matrix() if matrix is None else matrix
    gb = gaia_band(g)
    sel = np.where(matrix[:, 1] == 9.0)[0][:200]
    l_intep, ma_intep = interp1d(matrix[sel, 4], matrix[sel, 6]), interp1d(matrix[sel, 4], matrix[sel, 3])
    out = {k: [] for k in ('mags', 'dkep', 'pri_corr', 'sec_corr', 'logg', 'mass', 'lum')}
    for p in np.atleast_2d(theta):
        tt, rad, dist = sample_args(c, p, distance)
        lg = [float(orc.get_logg(t, matrix)) for t in tt]
        w, comp, stars = composite_plot(c, tt, lg, rad, dist, g['kepler_wl'])
        if c.nspec == 2:
            k = kepler_integrals(w, stars, g['kepler_wl'], g['kepler_tm'], 'trapz')
            pm, sm = -2.5 * np.log10(k[0]), -2.5 * np.log10(k[1])  # mft6.py:802
            gp = -2.5 * np.log10(gb.get_flux(w, stars[0])) - gb.Vega_zero_mag  # mft6.py:813
            gs = -2.5 * np.log10(gb.get_flux(w, stars[1])) - gb.Vega_zero_mag  # mft6.py:814
            gm = -2.5 * np.log10(gb.get_flux(w, comp) / gb.Vega_zero_flux)     # mft6.py:812
            out['mags'].append([pm, sm, gp, gs, gm])
            kc = sm - pm
            out['dkep'].append(kc)
            out['pri_corr'].append(np.sqrt(1 + 10 ** (-0.4 * kc)))
            out['sec_corr'].append(p[c.nspec + 2] * np.sqrt(1 + 10 ** (0.4 * kc)))
        else:
            k = kepler_integrals(w, stars, g['kepler_wl'], g['kepler_tm'], 'sum')
            out['mags'].append([-2.5 * np.log10(ks / np.array(ZP)) for ks in k])  # mft6.py:820-825
        out['logg'].append(lg)
        out['mass'].append([float(ma_intep(t)) for t in tt])
        out['lum'].append([float(l_intep(t)) for t in tt])
    return {k: np.array(v, dtype=float) for k, v in out.items() if v}


def window_parts(c, p, distance, g, matrix=None):
    """The window's wavelengths and [composite, star 0, star 1, (star 2)] on the plot=True window (the goldens store the
    stars' rows at ``win_idx``; the composite is their sum in star order)."""
    matrix = products_matrix() if matrix is None else matrix
    tt, rad, dist = sample_args(c, p, distance)
    lg = [float(orc.get_logg(t, matrix)) for t in tt]
    w, comp, stars = composite_plot(c, tt, lg, rad, dist, g['kepler_wl'])
    return w, [comp] + [s for s in stars]


def spectra(c, p, g, matrix=None):
    """[composite, star.., median-scaled composite] on the data pixels: reddened on the model grid, resampled
    (mft6.py:2394-2402), the composite scaled by median(data) / median(composite) (:2409)."""
    w, parts = window_parts(c, p, True, g, matrix)
    e = p[c.nspec]
    wl_um, spec = np.asarray(c.data[0]), np.asarray(c.data[1])
    rows = [interp1d(w, orc.extinct(w, s, e))(wl_um * 1e4) for s in parts]
    return np.array(rows + [rows[0] * (np.median(spec) / np.median(rows[0]))])


def _worst(name, got, want, absolute):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (name, got.shape, want.shape)
    d = np.abs(got - want) if absolute else np.abs(got - want) / np.abs(want)
    return float(np.max(d))


ABSOLUTE = ('mags', 'dkep', 'logg')  # magnitudes (a contrast may be 0) and log g: absolute; fluxes and factors: relative


def check_against(g, tol=1e-9):
    """Every array of the goldens against this module; returns the worst difference, asserts each within ``tol``."""
    cases = {'bin': (common.golden_case('B'), True), 'nod': (common.golden_case('A'), False), 'tri': (common.golden_case('C'), True)}
    worst = 0.0
    for tag, (c, distance) in cases.items():
        mine = evaluate(c, g[tag + '_theta'], distance, g)
        for k, v in mine.items():
            d = _worst(tag + '_' + k, v, g[tag + '_' + k], k in ABSOLUTE)
            assert d <= tol, (tag, k, d)
            worst = max(worst, d)
    idx = g['win_idx']
    for tag, key in (('bin', 'win_bin'), ('tri', 'win_tri')):
        c, distance = cases[tag]
        w, parts = window_parts(c, g[tag + '_theta'][0], distance, g)
        assert len(w) == int(g['win_len'][0]) and w[0] == g['win_wl_ends'][0] and w[-1] == g['win_wl_ends'][1]
        assert np.array_equal(parts[0], sum(parts[2:], parts[1]))  # mft6.py:744,751
        d = _worst(key, np.array([a[idx] for a in parts[1:]]), g[key], False)
        assert d <= tol, (key, d)
        worst = max(worst, d)
    cB, cA = cases['bin'][0], cases['nod'][0]
    for n, i in enumerate(g['specB_idx']):
        d = _worst('specB', spectra(cB, g['bin_theta'][int(i)], g), g['specB'][n], False)
        assert d <= tol, ('specB', n, d)
        worst = max(worst, d)
    d = _worst('specA', spectra(cA, g['specA_theta'][0], g), g['specA'][0], False)
    assert d <= tol, ('specA', d)
    return max(worst, d)
