#!/usr/bin/env python3
"""Pareto-smoothed importance sampling and the pointwise model checks on the device against a download plus their NumPy
definition, as JSON lines (and into --out, default profiles/psis_bench.jsonl), in one process on one GPU.
  * loo:    PSIS-LOO / WAIC / khat per observation (``psis.loo``) of 2,000 and of 7,500 samples on a 4,096 px problem built from
            golden case B's grid and bands.  device_ms: the call without the matrix.  The host side: matrix_call_ms, the same
            call handing back the pointwise matrix (n_obs x samples doubles: the download), and host_ms,
            ``psis.pointwise_stats`` on it.
  * series: PSIS of a resident log-weight series of 50 walkers x 15,000 rows (``psis.smooth_series``) against download_ms
            (``Series.read``) plus host_ms (``psis.series_weights``).
Every figure is the median of --reps calls (the host side: --host-reps) after a warm-up of both, the host's clock around the
synchronous call; the two sides are compared before they are timed (1e-9)."""
import argparse
import json
import os
import sys
import time

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'psis_bench.jsonl'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--host-reps', type=int, default=2)
    ap.add_argument('--samples', type=int, nargs='*', default=[2000, 7500])
    ap.add_argument('--rows', type=int, default=15000)
    a = ap.parse_args()
    import common
    import products_numpy as pn
    from mcmc_spec_amd import _lib, bands, psis, synth
    from mcmc_spec_amd.engine import Engine
    g = dict(np.load(pn.GOLDEN))
    c = common.golden_case('B')
    npix = 4096
    wl_um = synth.data_wavelengths_um(npix)
    flux = 1.0 + 0.1 * np.sin(np.arange(npix) / 37.0)
    eng = Engine(0)
    eng.stage_specs(c.specs)
    eng.stage_problem([wl_um, flux], 0.01 * flux, c.fr, [min(wl_um), max(wl_um)], c.ctm, c.ptm, c.tmi, c.tma, pn.products_matrix(), nspec=2,
                      bands=bands.make_bands(c.tables, *c.vega), tmin=c.tmin, tmax=c.tmax)
    gb = bands.Band('Gaia_G', g['gaia_wl'], g['gaia_tm'], float(g['gaia_zero_flux'][0]))
    gb.zero_mag = float(g['gaia_zero_mag'][0])
    eng.stage_products((g['kepler_wl'], g['kepler_tm']), gaia=gb, matrix=pn.products_matrix())
    lines = []

    def emit(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for n in a.samples:
        theta = synth.draw_walkers(n, seed=2, tmin=c.tmin, tmax=c.tmax)
        got = psis.loo(eng, theta)                                   # warm-up, and the comparison
        mat = psis.loo(eng, theta, pointwise=True)['pointwise']
        want = psis.pointwise_stats(mat)
        ok = np.isfinite(want['khat'])
        agree = float(max(np.max(np.abs(got['elpd_loo'] - want['elpd_loo']) / np.maximum(1.0, np.abs(want['elpd_loo']))),
                          np.max(np.abs(got['khat'][ok] - want['khat'][ok])) if ok.any() else 0.0))
        ms, _ = timed(lambda: psis.loo(eng, theta), a.reps)
        ms_m, res = timed(lambda: psis.loo(eng, theta, pointwise=True), a.host_reps)
        ms_h, _ = timed(lambda: psis.pointwise_stats(res['pointwise']), a.host_reps)
        host = float(np.median(ms_m) + np.median(ms_h))
        emit({'what': 'loo', 'samples': int(n), 'valid': int(got['count']), 'pixels': npix, 'observations': int(got['n_obs']),
              'tail_len': int(got['tail_len']), 'matrix_mb': float(mat.nbytes / 2 ** 20), 'reps': a.reps, 'host_reps': a.host_reps,
              'device_ms': float(np.median(ms)), 'device_ms_all': [float(x) for x in ms], 'matrix_call_ms': float(np.median(ms_m)),
              'host_ms': float(np.median(ms_h)), 'host_with_matrix_ms': host, 'ratio_host_over_device': host / float(np.median(ms)),
              'agreement': agree, 'n_bad_k': int(got['n_bad_k'])})

    nw = 50
    rng = np.random.default_rng(4)
    logw = 0.5 * rng.exponential(1.0, (a.rows, nw, 1)) - 4000.0       # Pareto weights of shape 0.5
    ser = _lib.Series(eng.ctx, nw, 1, cap_hint=a.rows)
    for b0 in range(0, a.rows, 1000):
        ser.append(logw[b0:b0 + 1000])
    w = _lib.Series(eng.ctx, nw, 1, cap_hint=a.rows)
    dev = lambda: psis.smooth_series(ser, a.rows, w)
    got = dev()
    want = psis.series_weights(logw[:, :, 0], got['tail_len'])
    agree = float(max(abs(got['khat'][0] - want['khat'][0]), abs(got['stats']['ess'][0] / want['stats']['ess'][0] - 1.0)))
    ms, _ = timed(dev, a.reps)
    ms_d, rows = timed(lambda: ser.read(0, a.rows), a.reps)
    ms_h, _ = timed(lambda: psis.series_weights(rows[:, :, 0], got['tail_len']), a.host_reps)
    host = float(np.median(ms_d) + np.median(ms_h))
    emit({'what': 'series', 'walkers': nw, 'rows': a.rows, 'samples': nw * a.rows, 'tail_len': int(got['tail_len'][0]), 'reps': a.reps,
          'host_reps': a.host_reps, 'device_ms': float(np.median(ms)), 'device_ms_all': [float(x) for x in ms],
          'download_ms': float(np.median(ms_d)), 'host_ms': float(np.median(ms_h)), 'host_with_download_ms': host,
          'ratio_host_over_device': host / float(np.median(ms)), 'agreement': agree, 'khat': float(got['khat'][0]),
          'ess': float(got['stats']['ess'][0])})
    ser.close()
    w.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
