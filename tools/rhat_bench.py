#!/usr/bin/env python3
"""What split R-hat and the moments cost on a resident series, as JSON lines (and into --out, default
profiles/rhat_bench.jsonl), in one process on one GPU.  Two shapes -- one chain of 50 walkers x 15,000 rows x 6 columns, and
8 members x 256 walkers x 15,000 rows x 6 -- and two sides that ALTERNATE inside every block after a warm-up of both:
  * device: msx_series_moments with the covariance (``Series.moments``), and without it (what ``get_rhat`` calls); a host
    clock around the synchronous call;
  * host: the download (``Series.read``) and then ``diagnostics.split_parts`` + ``diagnostics.moments`` on the array -- what
    a sampler without the device series' reductions would do with a resident chain.
A block is --reps alternations; the figures are the medians over the 3 blocks of each block's median.  The two results are
compared (1e-9 relative; covariances relative to the standard deviations)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, NDIM = 15000, 6
SHAPES = (('one chain', [50]), ('8 x 256', [256] * 8))
BLOCKS = 3


def clock(fn):
    t0 = time.perf_counter()
    res = fn()
    return 1e3 * (time.perf_counter() - t0), res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rhat_bench.jsonl'))
    ap.add_argument('--reps', type=int, default=3, help='alternations per block')
    ap.add_argument('--rows', type=int, default=ROWS)
    a = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process, see mcmc_spec_amd/_lib.py)
    from mcmc_spec_amd import _lib, diagnostics
    from mcmc_spec_amd.engine import Engine
    ctx = Engine(0).ctx
    lines = []
    for name, counts in SHAPES:
        nw = sum(counts)
        rng = np.random.default_rng(len(counts))
        ser = _lib.Series(ctx, nw, NDIM, counts, cap_hint=a.rows)
        centre, scale = np.array([5800.0, 3400.0, 0.3, 0.05, 0.02, 1e-4]), np.array([40.0, 60.0, 0.02, 0.01, 0.004, 2e-5])
        for b in range(0, a.rows, 1000):   # a random walk per walker and column, begun again every 1,000 rows: correlated rows
            m = min(1000, a.rows - b)
            x = centre + scale * np.cumsum(rng.normal(size=(m, nw, NDIM)), axis=0) / np.sqrt(m)
            ser.append(x)

        def host():
            t_read, rows = clock(lambda: ser.read(0, a.rows))
            t_calc, res = clock(lambda: (diagnostics.split_parts(rows, counts), diagnostics.moments(rows, counts)))
            return t_read, t_calc, res

        full = lambda: ser.moments(a.rows)
        lean = lambda: ser.moments(a.rows, cov=False)
        full(), lean(), host()   # warm-up: code objects, the scratch buffer, NumPy's pages
        blocks = {k: [] for k in ('device', 'device_no_cov', 'download', 'host')}
        dev = res = None
        for _ in range(BLOCKS):
            ms = {k: [] for k in blocks}
            for _ in range(a.reps):
                t, dev = clock(full)
                ms['device'].append(t)
                t, _ = clock(lean)
                ms['device_no_cov'].append(t)
                t_read, t_calc, res = host()
                ms['download'].append(t_read)
                ms['host'].append(t_calc)
            for k in blocks:
                blocks[k].append(float(np.median(ms[k])))
        parts, mo = res
        rel = lambda x, y: bool(np.all(np.abs(x - y) <= 1e-9 * np.abs(y)))
        sd = np.sqrt(np.diagonal(mo['cov'], axis1=1, axis2=2))
        agree = (all(rel(dev[k], parts[k]) for k in ('within', 'var_plus', 'between', 'rhat')) and rel(dev['mean'], mo['mean']) and
                 bool(np.all(np.abs(dev['cov'] - mo['cov']) <= 1e-9 * sd[:, :, None] * sd[:, None, :])))
        med = {k: float(np.median(v)) for k, v in blocks.items()}
        values = a.rows * nw * NDIM
        # bytes the device call reads: per column the two halves and the total, then the halves again for the deviations
        # (3 n'), and two columns for each of the 21 pairs
        streamed = 8 * a.rows * nw * (3 * NDIM + NDIM * (NDIM + 1))
        rec = {'what': 'rhat_moments', 'shape': name, 'members': len(counts), 'walkers': nw, 'rows': a.rows, 'ndim': NDIM, 'values': values,
               'reps': a.reps, 'blocks': BLOCKS, 'device_ms': med['device'], 'device_no_cov_ms': med['device_no_cov'],
               'download_ms': med['download'], 'host_ms': med['host'], 'host_with_download_ms': med['download'] + med['host'],
               'speedup_with_download': (med['download'] + med['host']) / med['device'],
               'speedup_no_cov_with_download': (med['download'] + med['host']) / med['device_no_cov'],
               'device_gb_per_s': streamed / (med['device'] * 1e-3) / 1e9, 'agree': agree, 'max_rhat': float(np.max(dev['rhat'])),
               'block_medians_ms': blocks}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        ser.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
