#!/usr/bin/env python3
"""Generate ``golden_products.npz``: what the REFERENCE's ``make_composite(..., plot=True)`` (mft6.py:786-828) returns for
chain samples, and what ``plot_results`` derives from it.  Runs only where the reference is checked out (see
make_golden.py, whose stub import and helpers this uses); the ``.npz`` is data and is what travels.

    python tests/golden/make_golden_products.py

What is the reference's own code, executed unmodified: ``make_composite`` with ``plot=True`` (window rule :663-687, the
Kepler integrals :792-799 / :820-822, the Gaia magnitudes :811-814), ``get_transmission('kepler', res)`` and
``('gaia,g', res)`` reading their tables from the reference's ``bps/`` (the call changes directory into the reference and
back: ``get_spec`` lists the model directory relative to the working directory), ``get_logg``, ``extinct``.

What is restated here, because it sits inside ``plot_results`` between plotting calls and cannot be called: the contrast
and the two correction factors (:2505, :2544-2545), the mass / luminosity look-ups (:2650, :2679, :2685-2690) and the
resampling of the sample spectra to the data pixels (:2394-2402, :2409) -- each a single NumPy / SciPy statement, copied.

UNPINNED, like all pyphot arithmetic here (make_golden.py): ``lib['Gaia_G']`` is a stub -- a photon-counting band built
from ``bps/gaia_g_pb.txt`` and the synthetic Vega per pyphot's published algorithm, with ``Vega_zero_mag =
-2.5 log10(Vega_zero_flux)``.
"""
import os
import sys
import warnings

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.dont_write_bytecode = True
warnings.filterwarnings('ignore')

import make_golden as mg  # noqa: E402
from mcmc_spec_amd import synth  # noqa: E402
from oracle import mft6_oracle as orc  # noqa: E402
import common  # noqa: E402
import products_numpy as pn  # noqa: E402

RES = 1700


def main():
    mft6 = mg.import_reference()
    teffs, loggs, wl, flux = common.golden_grid()
    specs = synth.grid_to_specs(teffs, loggs, wl, flux)
    matrix = pn.products_matrix()
    vega_w, vega_f = synth.synthetic_vega()
    bandlib = orc.make_band_library(synth.synthetic_band_tables(), vega_w, vega_f)

    orig_gt = mft6.get_transmission

    def get_transmission(f, res):  # the tables live in the reference's bps/, the (empty) model files in the scratch directory
        cwd = os.getcwd()
        os.chdir(mg.REF)
        try:
            return orig_gt(f, res)
        finally:
            os.chdir(cwd)

    mft6.get_transmission = get_transmission
    kep_w, kep_t, _, _ = get_transmission('kepler', RES)
    gaia_w, gaia_t, _, _ = get_transmission('gaia,g', RES)
    gaia = orc.OracleBand(gaia_w, gaia_t, vega_w, vega_f)
    bandlib['Gaia_G'] = gaia
    mg.patch_third_party(mft6, bandlib)
    stub = mft6.lib['Gaia_G']
    stub.Vega_zero_mag = -2.5 * np.log10(gaia.Vega_zero_flux)

    out = {'kepler_wl': np.array(kep_w), 'kepler_tm': np.array(kep_t), 'gaia_wl': np.array(gaia_w), 'gaia_tm': np.array(gaia_t),
           'gaia_zero_flux': np.array([gaia.Vega_zero_flux]), 'gaia_zero_mag': np.array([stub.Vega_zero_mag])}

    # the product isochrone's look-ups, mft6.py:2604-2605, :2650, :2679 (the matrix holds Teff and L as get_logg reads them)
    aage = matrix[:, 1]
    teff5, lum5, ma5 = matrix[:, 4][np.where(aage == 9.0)], matrix[:, 6][np.where(aage == 9.0)], matrix[:, 3][np.where(aage == 9.0)]
    l_intep = mft6.interp1d(teff5[:200], lum5[:200])
    ma_intep = mft6.interp1d(teff5[:200], ma5[:200])

    cwd = os.getcwd()
    os.chdir(mg.scratch_grid_dir(teffs, loggs))
    try:
        def run(c, theta, distance, tag):
            rows = {k: [] for k in ('mags', 'dkep', 'pri_corr', 'sec_corr', 'logg', 'mass', 'lum')}
            wins = []
            ns = c.nspec
            for p in theta:
                tt = list(p[:ns])
                lg = [mft6.get_logg(t, matrix) for t in tt]
                if distance:
                    rad, dist = list(p[ns + 1:2 * ns + 1]), p[2 * ns + 1]
                else:
                    rad, dist = list(p[ns + 2:2 * ns + 1]), False  # mft6.py:2498: [ratio1], False
                res = mft6.make_composite(tt, lg, rad, dist, c.fr[2], c.fr[5], c.r, specs, c.ctm, c.ptm, c.tmi, c.tma, None,
                                          nspec=ns, res=RES, plot=True)
                if ns == 2:
                    w, spe, pri_spec, sec_spec, pri_mag, sec_mag, gpm, gsm, gm = res
                    rows['mags'].append([pri_mag, sec_mag, gpm, gsm, gm])
                    kc = np.array(sec_mag - pri_mag)  # mft6.py:2505
                    rows['dkep'].append(kc)
                    rows['pri_corr'].append(np.sqrt(1 + 10 ** (-0.4 * kc)))  # mft6.py:2544
                    rows['sec_corr'].append(p[ns + 2] * np.sqrt(1 + 10 ** (0.4 * kc)))  # mft6.py:2504,:2545
                    wins.append((w, spe, pri_spec, sec_spec))
                else:
                    w, spe, s0, s1, s2, m0, m1, m2 = res
                    rows['mags'].append(np.array([m0, m1, m2]))  # each the six-element array the / zp list makes it
                    wins.append((w, spe, s0, s1, s2))
                rows['logg'].append([float(x) for x in lg])
                rows['mass'].append([float(ma_intep(t)) for t in tt])  # mft6.py:2685-2687
                rows['lum'].append([float(l_intep(t)) for t in tt])    # mft6.py:2689-2691
            out[tag + '_theta'] = np.array(theta)
            for k, v in rows.items():
                if v:
                    out[tag + '_' + k] = np.array(v, dtype=float)
            return wins

        cB, cA, cC = common.golden_case('B'), common.golden_case('A'), common.golden_case('C')
        g = cB.g
        # 12 binaries with distance: on-node T (3800), on-node g (3405: the matrix is flat at 5.0 there), both (3400), A_V = 0
        th = np.array(g['theta'][:12], dtype=float)
        th[1] = [3800.0, 3100.0, 0.106, 0.4994, 0.31, 2.0732e-3]
        th[2] = [3850.0, 3405.0, 0.0, 0.4994, 0.31, 2.0732e-3]
        th[3] = [3400.0, 3404.0, 0.2, 0.6, 0.5, 2.5e-3]
        th[4] = [3000.0, 4200.0, 0.05, 0.7, 0.9, 1.0e-3]   # the first and the last grid node
        winsB = run(cB, th, True, 'bin')
        # 6 binaries with distance=False on dataset A
        run(cA, np.vstack([th[:3], g['theta'][12:15]]), False, 'nod')
        # 6 triples on dataset B
        th3 = np.array(cC.theta[:6], dtype=float)
        th3[1, :3] = [3800.0, 3400.0, 3405.0]
        winsC = run(cC, th3, True, 'tri')

        # the raw window arrays of two samples, strided: every 61st sample, the first and last 16, 16 on either side of both
        # Kepler cut-offs (where the cut-off lies inside the window)
        w = winsB[0][0]
        idx = set(range(0, len(w), 61)) | set(range(16)) | set(range(len(w) - 16, len(w)))
        for edge in (min(kep_w), max(kep_w)):
            j = int(np.searchsorted(w, edge))
            idx |= set(range(max(0, j - 16), min(len(w), j + 16)))
        idx = np.array(sorted(idx))
        out['win_idx'] = idx.astype(np.int32)
        out['win_len'] = np.array([len(w)])
        out['win_wl_ends'] = np.array([w[0], w[-1]])
        # (the stars' rows: the composite is their elementwise sum in star order, mft6.py:744,751 -- bit for bit, asserted
        # here -- so storing it would add bytes and no information; the file has to stay below golden_reference.npz's size)
        assert np.array_equal(winsB[0][1], winsB[0][2] + winsB[0][3])
        assert np.array_equal(winsC[0][1], winsC[0][2] + winsC[0][3] + winsC[0][4])
        out['win_bin'] = np.array([a[idx] for a in winsB[0][2:]])
        out['win_tri'] = np.array([a[idx] for a in winsC[0][2:]])
        assert np.array_equal(winsC[0][0], w)

        # spectra of samples on the data pixels: mft6.py:2394-2402, :2409
        def spectra(c, p, win):
            ww, parts = win[0], win[1:]
            e = p[c.nspec]
            wl_um, spec = np.asarray(c.data[0]), np.asarray(c.data[1])
            rows = []
            for s in parts:
                s = mft6.extinct(ww, s, e)              # :2394-2396
                rows.append(mft6.interp1d(ww, s)(wl_um * 1e4))  # :2398-2402
            scaled = rows[0] * (np.median(spec) / np.median(rows[0]))  # :2409 (sspe *= ...)
            return np.array(rows + [scaled])

        out['specB_idx'] = np.array([0, 2, 5])
        out['specB'] = np.array([spectra(cB, th[i], winsB[i]) for i in (0, 2, 5)])
        # dataset A: its own window (other filters, other data range)
        winsA = []
        p = th[0]
        lg = [mft6.get_logg(t, matrix) for t in p[:2]]
        res = mft6.make_composite(list(p[:2]), lg, list(p[3:5]), p[5], cA.fr[2], cA.fr[5], cA.r, specs, cA.ctm, cA.ptm, cA.tmi,
                                  cA.tma, None, nspec=2, res=RES, plot=True)
        winsA.append(res[:4])
        out['specA'] = spectra(cA, p, winsA[0])[None]
        out['specA_theta'] = np.array([p])
        out['winA_wl_ends'] = np.array([res[0][0], res[0][-1], len(res[0])])
    finally:
        os.chdir(cwd)

    # the CPU twin against everything just written
    worst = pn.check_against(out)
    print('products_numpy vs reference: worst relative / absolute difference {:.3e}'.format(worst))
    path = os.path.join(HERE, 'golden_products.npz')
    np.savez_compressed(path, **out)
    print('wrote golden_products.npz ({} arrays, {:.0f} KiB)'.format(len(out), os.path.getsize(path) / 1024))


if __name__ == '__main__':
    main()
