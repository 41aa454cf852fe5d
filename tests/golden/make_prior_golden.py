#!/usr/bin/env python3
"""Generate tests/golden/golden_prior.npz: every branch of the reference's ``logprior`` on one shared walker set.

Runs only in the build container (needs ``/root/reference/mft6.py``), like ``make_golden.py``, whose helpers it
reuses (the stub import, the third-party stand-ins, the two-sample ``bayestar``).  The ``.npz`` is data and is what
travels::

    python tests/golden/make_prior_golden.py      # writes tests/golden/golden_prior.npz (byte-reproducible)

Per ndim (6: binary, 8: triple) one walker set ``thetaN`` is shared by all 32 flag combinations
ndim x dist_fit x ext x rad_prior x prior (0 or ``priorN``), under two A_V(distance) tables (``table`` 0: the
standard one; 1: a variant with zero-sigma bins, mft6.py:1237-1238).  The walkers:

  * random ones, drawn over a region wider than every branch's box, one coordinate at a time;
  * edge walkers: every gate bound of every branch (mft6.py:1227, 1229, 1286, 1347, 1411) exactly, and one
    ``np.nextafter`` step either side (A_V also at -0.0);
  * A_V-table walkers: 1 / plx exactly on a bin edge, below the first edge and beyond the last;
  * outside-isochrone walkers: a Teff inside a wide box (``tbox`` 1: ``tmin_wide`` / ``tmax_wide``) but outside the
    isochrone, so that ``rad_prior`` raises ValueError in get_radius after the gates pass.

``lpN[table, combo, walker]`` is the reference's value (NaN unless it returned a number) and ``codeN[...]`` the
outcome: 0 a value, 1 -inf, 2 returned None, 3 raised ValueError, 4 raised TypeError.  ``combosN[combo]`` =
(dist_fit, ext, rad_prior, has_prior).  ``avN_edges / avN_mu / avN_sig`` are the tables as the stub's samples
give them (np.mean / np.std of ``bayestar(...) * 3.1 * 0.884``, before the 0.05 substitution); ``avN_raw_*`` the
tables the stub was built from.

``postN_*``: a few reference ``logposterior`` values (ndim 6 on golden case B, ndim 8 on golden case C) per
(dist_fit, ext, rad_prior), with the list prior and the standard table; code 4 where it raised TypeError.
"""
import io
import itertools
import os
import sys
import warnings
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.dont_write_bytecode = True
warnings.filterwarnings('ignore')

import make_golden as mg  # noqa: E402
from mcmc_spec_amd import synth  # noqa: E402
from oracle import mft6_oracle as orc  # noqa: E402

OK, NEG_INF, NONE, VALUEERROR, TYPEERROR = 0, 1, 2, 3, 4
TMIN, TMAX = 3000.0, 4200.0
TMIN_WIDE, TMAX_WIDE = 2500.0, 7000.0  # wider than the isochrone's Teff span (2900 .. 6500)
PRIOR = {6: [3800.0, 0.0, 60.0, 50.0, 0.2, 0.1, 0.5, 0.3, 0.05, 0.04, 2.0732e-3, 0.0277e-3],
         8: [3800.0, 3400.0, 0.0, 60.0, 80.0, 1.0, 0.2, 0.1, 0.5, 0.4, 0.3, 0.05, 0.04, 0.03, 2.0e-3, 0.03e-3]}
BASE = {6: [3850.0, 3025.0, 0.3, 0.5, 0.31, 2.0732e-3],
        8: [3850.0, 3400.0, 3100.0, 0.3, 0.5, 0.4, 0.3, 2.0e-3]}
COMBOS = list(itertools.product((True, False), (True, False), (False, True), (False, True)))


def variant_table():
    edges, mu, sig = synth.make_av_table()
    sig = sig.copy()
    sig[::2] = 0.0  # every other bin: sigma 0 -> 0.05 in the reference (mft6.py:1237-1238)
    return edges, mu, sig


def exact_table(raw):
    """The (mu, sigma) the reference computes from the stub's two samples, bin by bin."""
    edges, mu, sig = raw
    mg.AV_EDGES, mg.AV_MU, mg.AV_SIG = raw
    m, s = [], []
    for b in range(len(mu)):
        g = mg.av_samples(0.5 * (edges[b] + edges[b + 1])) * 3.1 * 0.884
        m.append(np.mean(g))
        s.append(np.std(g))
    return np.asarray(edges, dtype=float), np.array(m), np.array(s)


def plx_on_edge(e):
    """A parallax whose reciprocal is exactly the distance e (None if no double near 1 / e has one)."""
    up = down = 1.0 / e
    for _ in range(8):
        for c in (up, down):
            if 1.0 / c == e:
                return float(c)
        up, down = np.nextafter(up, np.inf), np.nextafter(down, -np.inf)
    return None


def walker_set(ndim, rng, n_random=150):
    ns = (ndim - 2) // 2
    iav, ir1, iplx = ns, ns + 1, ndim - 1
    base = np.array(BASE[ndim])
    th, box = [], []
    # random walkers: each coordinate inside with probability 0.85, else over a wider range
    inner = [(3010.0, 4190.0)] * ns + [(0.06, 1.4), (0.06, 1.4)] + [(0.06, 1.0)] * (ns - 1) + [(1 / 900.0, 0.2)]
    wide = [(2950.0, 4250.0)] * ns + [(-0.1, 1.7), (-0.05, 1.7)] + [(-0.05, 1.2)] * (ns - 1) + [(-0.01, 0.3)]
    for _ in range(n_random):
        t = np.empty(ndim)
        for k in range(ndim):
            lo, hi = wide[k] if rng.random() < 0.15 else inner[k]
            t[k] = rng.uniform(lo, hi)
        th.append(t)
        box.append(0)

    def edge(k, v):
        for x in (v, np.nextafter(v, np.inf), np.nextafter(v, -np.inf)):
            t = base.copy()
            t[k] = x
            th.append(t)
            box.append(0)

    for s in range(ns):
        edge(s, TMIN)
        edge(s, TMAX)
    for k in range(ir1, ir1 + ns):
        edge(k, 0.05)
    edge(ir1, 1.5)
    for v in (0.0, 0.05, 1.5):
        edge(iav, v)
    t = base.copy()
    t[iav] = -0.0
    th.append(t)
    box.append(0)
    for v in (1 / 3000, 1 / 1000, 1 / 4, 0.0):
        edge(iplx, v)
    # the A_V table: 1 / plx on an edge (first, interior, last), below the first edge and beyond the last
    edges = synth.make_av_table()[0]
    for e in (edges[0], edges[1], edges[37], edges[80], edges[-1]):
        p = plx_on_edge(float(e))
        if p is not None:
            t = base.copy()
            t[iplx] = p
            th.append(t)
            box.append(0)
    for d in (3.5, 3500.0):
        t = base.copy()
        t[iplx] = 1.0 / d
        th.append(t)
        box.append(0)
    # outside the isochrone's Teff span, inside the wide box (the last one also fails the dist_fit parallax gate)
    for s, v, p in ((0, 2800.0, None), (ns - 1, 6800.0, None), (0, 6600.0, 0.5)):
        t = base.copy()
        t[s] = v
        if p is not None:
            t[iplx] = p
        th.append(t)
        box.append(1)
    t = base.copy()
    t[0] = 2950.0  # inside the isochrone and the wide box: a value
    th.append(t)
    box.append(1)
    return np.array(th), np.array(box, dtype=np.int8)


def outcome(fn):
    try:
        v = fn()
    except ValueError:
        return np.nan, VALUEERROR
    except TypeError:
        return np.nan, TYPEERROR
    if v is None:
        return np.nan, NONE
    v = float(v)
    if v == -np.inf:
        return v, NEG_INF
    return v, OK


def write_npz(path, out):
    """np.savez_compressed with a fixed member timestamp: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, 'w', compression=zipfile.ZIP_DEFLATED) as zf:
        for k in sorted(out):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(out[k]), allow_pickle=False)
            zi = zipfile.ZipInfo(k + '.npy', date_time=(1980, 1, 1, 0, 0, 0))
            zi.compress_type = zipfile.ZIP_DEFLATED
            zf.writestr(zi, buf.getvalue())


def main():
    mft6 = mg.import_reference()
    rng = np.random.default_rng(2024)
    matrix = synth.make_isochrone_matrix()
    vega_w, vega_f = synth.synthetic_vega()
    bandlib = orc.make_band_library(synth.synthetic_band_tables(), vega_w, vega_f)
    mg.patch_third_party(mft6, bandlib)
    raw = [synth.make_av_table(), variant_table()]
    out = {'tmin': np.array([TMIN, TMIN_WIDE]), 'tmax': np.array([TMAX, TMAX_WIDE]),
           'combo_fields': np.array(['dist_fit', 'ext', 'rad_prior', 'has_prior'])}
    for ndim in (6, 8):
        ns = (ndim - 2) // 2
        th, box = walker_set(ndim, rng)
        out['theta%d' % ndim], out['tbox%d' % ndim], out['prior%d' % ndim] = th, box, np.array(PRIOR[ndim])
        out['combos%d' % ndim] = np.array(COMBOS, dtype=np.int8)
        lp = np.full((2, len(COMBOS), len(th)), np.nan)
        code = np.zeros((2, len(COMBOS), len(th)), dtype=np.int8)
        for ti, tab in enumerate(raw):
            e, m, s = exact_table(tab)
            out['av%d_edges' % ti], out['av%d_mu' % ti], out['av%d_sig' % ti] = e, m, s
            out['av%d_raw_mu' % ti], out['av%d_raw_sig' % ti] = tab[1], tab[2]
            mg.AV_EDGES, mg.AV_MU, mg.AV_SIG = tab
            for ci, (df, ext, rp, hp) in enumerate(COMBOS):
                prior = list(PRIOR[ndim]) if hp else 0
                for i, t in enumerate(th):
                    lo, hi = out['tmin'][box[i]], out['tmax'][box[i]]
                    lp[ti, ci, i], code[ti, ci, i] = outcome(lambda: mft6.logprior(
                        list(t), ns, 0, lo, hi, matrix, 10.0, 20.0, prior=prior, ext=ext, dist_fit=df, rad_prior=rp))
        out['lp%d' % ndim], out['code%d' % ndim] = lp, code
        print('ndim {}: {} walkers; outcomes {}'.format(ndim, len(th), np.bincount(code.ravel(), minlength=5)))

    # ---- a few whole posteriors: ndim 6 on golden case B, ndim 8 on golden case C (standard A_V table)
    mg.AV_EDGES, mg.AV_MU, mg.AV_SIG = raw[0]
    g = np.load(os.path.join(HERE, 'golden_reference.npz'))
    teffs, loggs = np.arange(3000, 4300, 100), np.array([4.0, 4.5, 5.0, 5.5])
    wl = np.arange(5000, 24000, 0.2)
    specs = synth.grid_to_specs(teffs, loggs, wl, synth.make_grid(teffs, loggs, wl, nlines=1500, seed=11))
    ctm, ptm = synth.synthetic_contrast_filters(), synth.synthetic_phot_filters()
    tmi = min(min(w) for tm in (ctm, ptm) for w in tm[0])  # make_golden.py's tm_extrema
    tma = max(max(w) for tm in (ctm, ptm) for w in tm[0])
    data, err = [g['B_wl'], g['B_flux']], g['B_err']
    r = [min(data[0]), max(data[0])]
    pnames = np.array(['sdss,r', 'sdss,i', 'sdss,z', 'j', 'h', 'k'])
    frB = [synth.EXAMPLE_CMAG, synth.EXAMPLE_CERR, np.array(['lp600', 'Kp']), np.array(synth.EXAMPLE_PMAG),
           synth.EXAMPLE_PERR, pnames]
    frC = [[2.08, 1.3, 3.1, 2.2], [0.14, 0.02, 0.2, 0.05], np.array(['lp600', 'Kp', 'lp600', 'Kp']),
           np.array(synth.EXAMPLE_PMAG), synth.EXAMPLE_PERR, pnames]
    ctm4 = [x + x for x in ctm]
    post_theta = {6: np.array([BASE[6], [3600.0, 3200.0, 0.6, 0.7, 0.5, 3.0e-3], [3850.0, 3025.0, 0.3, 0.5, 0.04, 2.0732e-3]]),
                  8: np.array([BASE[8], [3700.0, 3300.0, 3050.0, 0.6, 0.6, 0.5, 0.4, 3.0e-3]])}
    setup = {6: (frB, ctm), 8: (frC, ctm4)}
    cwd = os.getcwd()
    os.chdir(mg.scratch_grid_dir(teffs, loggs))  # get_spec parses the grid's file names (make_golden.py)
    for ndim in (6, 8):
        ns = (ndim - 2) // 2
        fr, ct = setup[ndim]
        combos = list(itertools.product((True, False), (True, False), (False, True)))
        vals = np.full((len(combos), len(post_theta[ndim])), np.nan)
        codes = np.zeros(vals.shape, dtype=np.int8)
        for ci, (df, ext, rp) in enumerate(combos):
            for i, t in enumerate(post_theta[ndim]):
                vals[ci, i], codes[ci, i] = outcome(lambda: mft6.logposterior(
                    list(t), fr, ns, 0, data, err, 1700, r, specs, ct, ptm, tmi, tma, None, TMIN, TMAX, matrix, 10.0,
                    20.0, prior=list(PRIOR[ndim]), a=ext, dist_fit=df, rad_prior=rp))
        out['post%d_theta' % ndim], out['post%d_combos' % ndim] = post_theta[ndim], np.array(combos, dtype=np.int8)
        out['post%d_value' % ndim], out['post%d_code' % ndim] = vals, codes
        print('ndim {} posteriors: outcomes {}'.format(ndim, np.bincount(codes.ravel(), minlength=5)))
    os.chdir(cwd)
    path = os.path.join(HERE, 'golden_prior.npz')
    write_npz(path, out)
    print('wrote {} ({} bytes)'.format(path, os.path.getsize(path)))


if __name__ == '__main__':
    main()
