#!/usr/bin/env python3
"""The posterior predictive check on the device against what a user does without it, as JSON lines
(and into --out), in one process on one GPU, on a 4,096 px problem built from golden case B's grid and bands:
  * draw:  2,000 samples, the reference's own draw (mft6.py:2486), through msx_predictive_batch from host memory;
  * chain: a resident 50-walker x 15,000-row chain thinned by --thin (50 x 150 = 7,500 samples at the default 100)
           through msx_series_predictive, no copy of the chain.
device_ms: band + quantiles (0.16, 0.5, 0.84) + residuals + terms in ONE call, the host's clock around the synchronous call
(copies of the samples and of the results included), the median and the spread of --reps calls after a warm-up.
baseline_ms: the same numbers the way they are had without this call -- ``products.spectra`` in chunks of --chunk samples, the
download, ``products.evaluate`` for the band terms, then tests/predictive_numpy.py (np.mean / var / min / max / quantile;
norm_spec and chisq per sample) -- the median of --baseline-reps runs.  The two are compared before they are timed
(agreement: the worst relative difference of the means and of chi_total).  sclk_mhz: the shader clock read right after the
timed device calls (None where the platform does not report it): the clock the numbers were taken at."""
import argparse
import json
import os
import subprocess
import sys
import time
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def timed(fn, reps):
    ms, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms, res


def shader_clock_mhz():
    """The current shader clock, read (never set) from rocm-smi; None where that does not work."""
    try:
        out = subprocess.run(['rocm-smi', '-d', '0', '--showclocks', '--json'], capture_output=True, text=True, timeout=20).stdout
        for card in json.loads(out).values():
            for key, val in card.items():
                if 'sclk' in key.lower() and 'mhz' in str(val).lower():
                    return float(str(val).lower().replace('(', ' ').replace('mhz', ' ').split()[0])
    except Exception:  # noqa: BLE001 - a missing tool or another format: not measured
        return None
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--baseline-reps', type=int, default=2)
    ap.add_argument('--chunk', type=int, default=250)
    ap.add_argument('--thin', type=int, default=100)
    ap.add_argument('--rows', type=int, default=15000)
    ap.add_argument('--draw', type=int, default=2000)
    a = ap.parse_args()
    import common
    import predictive_numpy as twin
    import products_numpy as pn
    from mcmc_spec_amd import _lib, bands, predictive, products, synth
    from mcmc_spec_amd.engine import Engine
    g = dict(np.load(pn.GOLDEN))
    c = common.golden_case('B')
    npix = 4096
    wl_um = synth.data_wavelengths_um(npix)
    flux = 1.0 + 0.1 * np.sin(np.arange(npix) / 37.0)
    c4 = types.SimpleNamespace(**{k: getattr(c, k) for k in ('nspec', 'fr', 'ctm', 'ptm', 'tmi', 'tma', 'specs', 'bandlib')})
    c4.data, c4.r, c4.err = [wl_um, flux], [min(wl_um), max(wl_um)], 0.01 * flux
    eng = Engine(0)
    eng.stage_specs(c.specs)
    eng.stage_problem(c4.data, c4.err, c.fr, c4.r, c.ctm, c.ptm, c.tmi, c.tma, pn.products_matrix(), nspec=2,
                      bands=bands.make_bands(c.tables, *c.vega), tmin=c.tmin, tmax=c.tmax)
    gb = bands.Band('Gaia_G', g['gaia_wl'], g['gaia_tm'], float(g['gaia_zero_flux'][0]))
    gb.zero_mag = float(g['gaia_zero_mag'][0])
    eng.stage_products((g['kepler_wl'], g['kepler_tm']), gaia=gb, matrix=pn.products_matrix())
    nc, nph = len(c.fr[2]), len(c.fr[5])
    band_cols = ['contrast:{}'.format(f) for f in range(nc)] + ['phot:{}'.format(p) for p in range(nph)]
    q = (0.16, 0.5, 0.84)
    lines = []

    def baseline(theta):
        S = np.concatenate([products.spectra(eng, theta[i:i + a.chunk])[0] for i in range(0, len(theta), a.chunk)])
        b = products.evaluate(eng, theta, band_cols)
        return twin.check(c4, theta, S, b[:, :nc], b[:, nc:], q)

    def record(what, theta, device, extra):
        got = device()   # warm-up, and the comparison
        ms, _ = timed(device, a.reps)
        clk = shader_clock_mhz()
        ms_b, want = timed(lambda: baseline(theta), a.baseline_reps)
        agree = float(max(np.max(np.abs(got['mean'] / want['mean'] - 1)), np.max(np.abs(got['z2_mean'] / want['z2_mean'] - 1))))
        exact = bool(np.array_equal(got['quantiles'], want['quantiles']) and np.array_equal(got['min'], want['min']))
        rec = {'what': what, 'samples': int(len(theta)), 'pixels': npix, 'valid': int(got['count']), 'device_ms': float(np.median(ms)),
               'device_ms_min': float(np.min(ms)), 'device_ms_max': float(np.max(ms)), 'device_ms_all': [float(x) for x in ms],
               'baseline_ms': float(np.median(ms_b)), 'baseline_ms_all': [float(x) for x in ms_b], 'baseline_chunk': a.chunk,
               'ratio_baseline_over_device': float(np.median(ms_b) / np.median(ms)), 'agreement': agree, 'quantiles_and_min_exact': exact,
               'sclk_mhz': clk}
        rec.update(extra)
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    theta = synth.draw_walkers(a.draw, seed=2, tmin=c.tmin, tmax=c.tmax)
    record('draw', theta, lambda: predictive.check(eng, theta, q), {})

    nw = 50
    x = synth.draw_walkers(nw * a.rows, seed=3, tmin=c.tmin, tmax=c.tmax).reshape(a.rows, nw, 6)
    ser = _lib.Series(eng.ctx, nw, 6, cap_hint=a.rows)
    for b0 in range(0, a.rows, 1000):
        ser.append(x[b0:b0 + 1000])
    record('chain', x[::a.thin].reshape(-1, 6), lambda: predictive.check_series(ser, a.rows, [eng], q, 0, a.thin)[0],
           {'walkers': nw, 'rows': a.rows, 'thin': a.thin, 'resident': True})
    ser.close()
    if a.out:
        with open(a.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
