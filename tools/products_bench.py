#!/usr/bin/env python3
"""Derived posteriors on the device against the NumPy twin of the reference's loop, as JSON lines
(and into --out), in one process on one GPU, on golden case B (700 px, six photometric bands) with the Kepler and Gaia
curves of tests/golden/golden_products.npz:
  * batch: the reference's workload -- 2,000 samples, all its derived columns (products.REFERENCE_COLUMNS) -- through
    msx_products_batch from host memory (the copies included), and the kernel alone between two events
    (msx_products_batch_dev on device buffers);
  * chain: the whole 50 x 15,000 chain through msx_series_derive plus the 16 / 50 / 84 of three columns;
  * spectra: 100 samples' spectra at 4,096 px with the median scale (msx_products_spectra, copies included) against the
    twin's spectra on --host-samples samples;
  * host: tests/products_numpy.py on --host-samples samples (each runs the composite over the plot=True window, as the
    reference does), scaled to the workload's sample count -- host_ms is an extrapolation and says so.
Device: the median and the spread (min, max) of --reps calls after a warm-up.  kernel_ms is measured on the device, between
two events around the launch on device buffers; every wall_ms is the host's clock around a synchronous call, host-to-device
and device-to-host copies included, and is labelled so.  The first values are compared with the twin's."""
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
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--host-samples', type=int, default=8)
    a = ap.parse_args()
    import torch
    import common
    import products_numpy as pn
    from mcmc_spec_amd import _lib, bands, products, summary, synth
    from mcmc_spec_amd.engine import Engine
    g = dict(np.load(pn.GOLDEN))
    c = common.golden_case('B')
    eng = Engine(0)
    eng.stage_specs(c.specs)
    eng.stage_problem(c.data, c.err, c.fr, c.r, c.ctm, c.ptm, c.tmi, c.tma, pn.products_matrix(), nspec=2,
                      bands=bands.make_bands(c.tables, *c.vega), tmin=c.tmin, tmax=c.tmax)
    gb = bands.Band('Gaia_G', g['gaia_wl'], g['gaia_tm'], float(g['gaia_zero_flux'][0]))
    gb.zero_mag = float(g['gaia_zero_mag'][0])
    eng.stage_products((g['kepler_wl'], g['kepler_tm']), gaia=gb, matrix=pn.products_matrix())
    cols = products.columns(products.REFERENCE_COLUMNS)
    lines = []

    def out(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    def spread(ms):
        return {'wall_ms': float(np.median(ms)), 'wall_ms_min': float(np.min(ms)), 'wall_ms_max': float(np.max(ms)),
                'wall_ms_all': [float(x) for x in ms]}

    # ---- host: the twin on a few samples ----
    th_host = synth.draw_walkers(a.host_samples, seed=1, tmin=c.tmin, tmax=c.tmax)
    t0 = time.perf_counter()
    ref = pn.evaluate(c, th_host, True, g)
    host_ms_per_sample = 1e3 * (time.perf_counter() - t0) / a.host_samples
    got = products.evaluate(eng, th_host, ['kep_contrast', 'pri_corr', 'sec_corr'])
    agree = float(max(np.max(np.abs(got[:, 0] - ref['dkep'])), np.max(np.abs(got[:, 1] / ref['pri_corr'] - 1)),
                      np.max(np.abs(got[:, 2] / ref['sec_corr'] - 1))))

    # ---- batch: 2,000 samples, the reference's columns ----
    n = 2000
    theta = synth.draw_walkers(n, seed=2, tmin=c.tmin, tmax=c.tmax)
    products.evaluate(eng, theta, cols)   # warm-up
    ms, _ = timed(lambda: products.evaluate(eng, theta, cols), a.reps)
    d_theta = torch.tensor(theta, device='cuda:0')
    d_cols = torch.tensor(np.asarray(cols, dtype=np.int64), device='cuda:0').to(torch.int32)
    d_out = torch.empty((n, len(cols)), dtype=torch.float64, device='cuda:0')
    d_status = torch.empty(n, dtype=torch.int32, device='cuda:0')
    stream = torch.cuda.current_stream()
    kernel_ms = []
    for i in range(a.reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        eng.ctx.products_batch_dev(d_theta.data_ptr(), n, 6, d_cols.data_ptr(), len(cols), d_out.data_ptr(), d_status.data_ptr(),
                                   stream.cuda_stream)
        e1.record(stream)
        e1.synchronize()
        if i:
            kernel_ms.append(e0.elapsed_time(e1))
    rec = {'what': 'batch', 'samples': n, 'columns': len(cols), 'agreement_with_twin': agree,
           'host_ms_per_sample': host_ms_per_sample, 'host_ms_extrapolated': host_ms_per_sample * n, 'host_samples_timed': a.host_samples,
           'kernel_ms': float(np.median(kernel_ms)), 'kernel_ms_min': float(np.min(kernel_ms)), 'kernel_ms_max': float(np.max(kernel_ms))}
    rec.update(spread(ms))
    out(rec)

    # ---- chain: 50 walkers x 15,000 rows through derive, then the 16 / 50 / 84 ----
    nw, rows = 50, 15000
    x = synth.draw_walkers(nw * rows, seed=3, tmin=c.tmin, tmax=c.tmax).reshape(rows, nw, 6)
    ser = _lib.Series(eng.ctx, nw, 6, cap_hint=rows)
    for b in range(0, rows, 1000):
        ser.append(x[b:b + 1000])
    three = products.columns(['kep_contrast', 'pri_corr', 'sec_corr'])
    dst = _lib.Series(eng.ctx, nw, 3, cap_hint=rows)

    def chain():
        products.derive(ser, [eng], three, rows, dst=dst)
        return summary.summary_of(dst, rows, (0.16, 0.5, 0.84))

    chain()
    ms, summ = timed(chain, a.reps)
    ms_d, _ = timed(lambda: products.derive(ser, [eng], three, rows, dst=dst), a.reps)
    rec = {'what': 'chain', 'walkers': nw, 'rows': rows, 'samples': nw * rows, 'columns': 3, 'derive_wall_ms': float(np.median(ms_d)),
           'host_ms_per_sample': host_ms_per_sample, 'host_ms_extrapolated': host_ms_per_sample * nw * rows,
           'dkep_16_50_84': [float(v) for v in summ['quantiles'][0, 0]]}
    rec.update(spread(ms))
    out(rec)
    ser.close()
    dst.close()

    # ---- spectra: 100 samples at 4,096 px ----
    import types
    wl_um = synth.data_wavelengths_um(4096)
    flux = 1.0 + 0.1 * np.sin(np.arange(4096) / 37.0)
    c4 = types.SimpleNamespace(**{k: getattr(c, k) for k in ('nspec', 'fr', 'ctm', 'ptm', 'tmi', 'tma', 'specs', 'bandlib')})
    c4.data, c4.r = [wl_um, flux], [min(wl_um), max(wl_um)]
    eng4 = Engine(0)
    eng4.stage_specs(c.specs)
    eng4.stage_problem(c4.data, 0.01 * flux, c.fr, c4.r, c.ctm, c.ptm, c.tmi, c.tma, pn.products_matrix(), nspec=2,
                       bands=bands.make_bands(c.tables, *c.vega), tmin=c.tmin, tmax=c.tmax)
    eng4.stage_products((g['kepler_wl'], g['kepler_tm']), gaia=gb, matrix=pn.products_matrix())
    th100 = synth.draw_walkers(100, seed=4, tmin=c.tmin, tmax=c.tmax)
    products.spectra(eng4, th100)
    ms, (spec, scale) = timed(lambda: products.spectra(eng4, th100), a.reps)
    t0 = time.perf_counter()
    ref = [pn.spectra(c4, p, g) for p in th100[:a.host_samples]]
    host_ms = 1e3 * (time.perf_counter() - t0) / a.host_samples
    agree = float(max(np.max(np.abs(spec[i, 0] / ref[i][-1] - 1)) for i in range(a.host_samples)))
    rec = {'what': 'spectra', 'samples': 100, 'pixels': 4096, 'agreement_with_twin': agree, 'host_ms_per_sample': host_ms,
           'host_ms_extrapolated': host_ms * 100, 'host_samples_timed': a.host_samples}
    rec.update(spread(ms))
    out(rec)
    if a.out:
        with open(a.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
