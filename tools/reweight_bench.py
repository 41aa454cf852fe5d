#!/usr/bin/env python3
"""What importance reweighting costs on a resident series, as JSON lines (and into --out, default
profiles/reweight_bench.jsonl), in one process on one GPU.  One chain of 50 walkers x 15,000 rows x 6 columns around golden
case B's theta on a 4,096-pixel spectrum, and a second engine holding the same problem under a parallax prior moved by half
its width.  Two records, each with two sides that ALTERNATE inside every block after a warm-up of both:
  * rescore: the chain scored under both engines on the device (2 x msx_series_logprob) and the log-weight formed
    (msx_series_lincomb), against the download (``Series.read``) followed by both engines' host-pointer ``logposterior`` of
    the flat chain and the subtraction;
  * reduce: msx_series_weights, msx_series_wmoments (mean and covariance of the six columns) and msx_series_resample with
    nout = N, against the download of the chain and the log-weights followed by the NumPy definition of the three
    (``reweight.weights`` / ``weight_stats`` / ``wmoments`` / ``resample``).
A block is --reps alternations; the figures are the medians over the 3 blocks of each block's median.  The results of the
two sides are compared: the log-weights, the statistics, the moments and the drawn indices bit for bit (the definition is fed
the device's weights), the weights to the ulp distance recorded."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

BLOCKS = 3


def clock(fn):
    t0 = time.perf_counter()
    res = fn()
    return 1e3 * (time.perf_counter() - t0), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'reweight_bench.jsonl'))
    ap.add_argument('--reps', type=int, default=3, help='alternations per block')
    ap.add_argument('--rows', type=int, default=15000)
    ap.add_argument('--walkers', type=int, default=50)
    ap.add_argument('--npix', type=int, default=4096)
    a = ap.parse_args()
    import common
    from mcmc_spec_amd import _lib, bands, reweight, synth
    from mcmc_spec_amd.engine import Engine
    c = common.golden_case('B')
    wl_um = synth.data_wavelengths_um(a.npix)
    flux = 1.0 + 0.1 * np.sin(np.arange(a.npix) / 37.0)
    engines = []
    for shift in (0.0, 0.5):
        prior = list(c.prior)
        prior[-2] += shift * prior[-1]
        eng = Engine(0)
        eng.stage_specs(c.specs)
        eng.stage_problem([wl_um, flux], 0.01 * flux, c.fr, [min(wl_um), max(wl_um)], c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=2,
                          bands=bands.make_bands(c.tables, *c.vega), av_table=common.av_table_exact(), tmin=c.tmin, tmax=c.tmax,
                          prior=prior)
        engines.append(eng)
    old, new = engines
    nw, rows = a.walkers, a.rows
    N = nw * rows
    sc = np.array([30.0, 30.0, 0.02, 0.02, 0.02, 2e-5]) * 0.3
    x = c.theta[0] + np.random.default_rng(3).normal(size=(rows, nw, 6)) * sc
    ser = _lib.Series(old.ctx, nw, 6, cap_hint=rows)
    for b0 in range(0, rows, 1000):
        ser.append(x[b0:b0 + 1000])
    lines = []

    def blocks_of(sides):
        for fn in sides.values():
            fn()                                  # warm-up: code objects, scratch buffers, NumPy's pages
        med, last = {k: [] for k in sides}, {}
        for _ in range(BLOCKS):
            ms = {k: [] for k in sides}
            for _ in range(a.reps):
                for k, fn in sides.items():
                    t, last[k] = clock(fn)
                    ms[k].append(t)
            for k in sides:
                med[k].append(float(np.median(ms[k])))
        return {k: float(np.median(v)) for k, v in med.items()}, med, last

    # ---- the re-score under two engines ------------------------------------------------------------------------------------
    def device_rescore():
        lp_new, lp_old = reweight.rescore(ser, rows, [new]), reweight.rescore(ser, rows, [old])
        logw = reweight.log_weights([(lp_new, 0, 1.0), (lp_old, 0, -1.0)])
        lp_new.close()
        lp_old.close()
        return logw

    def host_rescore():
        flat = ser.read(0, rows).reshape(-1, 6)
        lp_new, lp_old = (e.ctx.logprob_batch(flat, _lib.MODE_LOGPOST)[0] for e in (new, old))
        return (1.0 * lp_new + -1.0 * lp_old).reshape(rows, nw)

    keep = []

    def device_side():
        keep.append(device_rescore())
        while len(keep) > 1:
            keep.pop(0).close()
        return keep[-1]

    med, all_ms, last = blocks_of({'device': device_side, 'host': host_rescore})
    logw_dev = last['device'].read(0, rows)[:, :, 0]
    rec = {'what': 'rescore', 'walkers': nw, 'rows': rows, 'ndim': 6, 'pixels': a.npix, 'samples': N, 'engines': 2, 'reps': a.reps,
           'blocks': BLOCKS, 'device_ms': med['device'], 'download_and_host_pointer_batches_ms': med['host'],
           'ratio': med['host'] / med['device'], 'evaluations_per_s_device': 2 * N / (med['device'] * 1e-3),
           'logw_bit_for_bit': bool(np.array_equal(logw_dev, last['host'], equal_nan=True)),
           'finite': int(np.isfinite(logw_dev).sum()), 'block_medians_ms': all_ms}
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    logw = last['device']

    # ---- weights, weighted moments, resampling -----------------------------------------------------------------------------
    w = _lib.Series(old.ctx, nw, 1, cap_hint=rows)
    dst = [_lib.Series(old.ctx, 1, 6, cap_hint=N)]

    def device_reduce():
        st = logw.weights(rows, w)
        mo = ser.wmoments(w, rows)
        idx = ser.resample(w, rows, [N], dst, seed=1)
        return st, mo, idx

    def host_reduce():
        t_read, (xx, lw) = clock(lambda: (ser.read(0, rows), logw.read(0, rows)[:, :, 0]))
        ww = reweight.weights(lw)
        st = reweight.weight_stats(lw, ww)
        mo = reweight.wmoments(xx, ww)
        out, idx = reweight.resample(xx, ww, [N], seed=1)
        return t_read, st, mo, idx, out

    med, all_ms, last = blocks_of({'device': device_reduce, 'host': host_reduce})
    st, mo, idx = last['device']
    wd = w.read(0, rows)[:, :, 0]
    lw = logw.read(0, rows)[:, :, 0]
    ref_w = reweight.weights(lw)
    ulp = int(np.abs(wd.view(np.int64) - np.ascontiguousarray(ref_w).view(np.int64)).max())
    st2, mo2 = reweight.weight_stats(lw, wd), reweight.wmoments(x, wd)
    rows2, idx2 = reweight.resample(x, wd, [N], seed=1)
    exact = (all(np.array_equal(st[k], st2[k]) for k in st2) and all(np.array_equal(mo[k], mo2[k]) for k in mo2) and
             np.array_equal(idx[0], idx2[0]) and np.array_equal(dst[0].read()[:, 0, :], rows2[0]))
    rec = {'what': 'weights_wmoments_resample', 'walkers': nw, 'rows': rows, 'ndim': 6, 'samples': N, 'nout': N, 'reps': a.reps,
           'blocks': BLOCKS, 'device_ms': med['device'], 'download_and_definition_ms': med['host'], 'download_ms': float(last['host'][0]),
           'ratio': med['host'] / med['device'], 'ess': float(st['ess'][0]), 'nbad': int(st['nbad'][0]), 'nzero': int(st['nzero'][0]),
           'weights_max_ulp_to_numpy_exp': ulp, 'bit_for_bit_given_the_weights': bool(exact), 'distinct_drawn': int(np.unique(idx[0]).size),
           'block_medians_ms': all_ms}
    print(json.dumps(rec), flush=True)
    lines.append(rec)
    for s in [ser, w, logw] + dst:
        s.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for r in lines:
                f.write(json.dumps(r) + '\n')


if __name__ == '__main__':
    main()
