#!/usr/bin/env python3
"""Posterior summaries on the device against the NumPy computations they replace, as JSON lines
(and into --out), in one process on one GPU.  For each shape -- 50 walkers x 15,000 rows x 6 (the reference's), 8 members
x 50 x 15,000, 1,024 x 15,000 -- on AR(1) rows (rho 0.9, as tools/autocorr_bench.py makes them) in which every walker
repeats its previous row with probability 0.3 (ties, as a chain has them):
  * quantiles: summary.quantiles (0.16 / 0.5 / 0.84, all columns) against np.quantile on the flat chain;
  * marginals: summary.marginals (T1, T2, R1, R2 and R2 / R1, 75 edges, the reference's rule) against the searchsorted
    restatement of the reference's loop (tests/summary_numpy.py), min / max / linspace / the ratio included;
  * corner_counts: 6 columns, 50 bins, against np.histogram and np.histogram2d on the flat chain.
Device: the median of --reps calls after a warm-up; host: the best of up to 3.  Every device result is compared with the
host's (exact).  stream_bytes: what the device call's passes read (N x 8 per pass and column read)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SHAPES = [(1, 50, 15000), (8, 50, 15000), (1, 1024, 15000)]    # members, walkers per member, rows
CENTER = np.array([3500.0, 3300.0, 0.3, 1.0, 0.8, 1e-3])
SCALE = np.array([30.0, 30.0, 0.02, 0.02, 0.02, 2e-5])
Q = [0.16, 0.5, 0.84]
SEL_PASSES = 8     # csrc/summary_kernels.h: kSelPasses


def rows_with_ties(n, nw, ndim, rho, repeat, seed):
    rng = np.random.default_rng(seed)
    x = np.empty((n, nw, ndim))
    x[0] = rng.normal(size=(nw, ndim))
    s = np.sqrt(1.0 - rho * rho)
    for t in range(1, n):
        x[t] = rho * x[t - 1] + s * rng.standard_normal((nw, ndim))
        keep = rng.random(nw) < repeat
        x[t][keep] = x[t - 1][keep]
    return x * SCALE + CENTER


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
    ap.add_argument('--reps', type=int, default=5)
    a = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process, see mcmc_spec_amd/_lib.py)
    from mcmc_spec_amd import _lib, summary
    from summary_numpy import flat_members, numpy_counts2d, reference_counts
    ctx = _lib.Context(0)
    ratio = summary.col_ratio(4, 3)
    mcols = [0, 1, 3, 4, ratio]
    lines = []

    def out(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for k, wpm, n in SHAPES:
        nw = k * wpm
        x = rows_with_ties(n, nw, 6, 0.9, 0.3, seed=nw + n)
        counts = [wpm] * k
        ser = _lib.Series(ctx, nw, 6, counts, cap_hint=n)
        for b in range(0, n, 1000):
            ser.append(x[b:b + 1000])
        flats = flat_members(x, n, 0, 1, counts)
        total = n * nw
        host_reps = 3 if total < 2e6 else 1

        def host_quantiles():
            return np.stack([np.quantile(f, Q, axis=0).T for f in flats])

        def host_marginals():
            res = []
            for f in flats:
                for c in mcols:
                    v = f[:, 4] / f[:, 3] if c == ratio else f[:, c]
                    e = np.linspace(v.min(), v.max(), 75)
                    res.append(reference_counts(v, e))
            return np.array(res).reshape(k, len(mcols), 75)

        def host_corner():
            c1, c2 = [], []
            for f in flats:
                edges = []
                for j in range(6):
                    h, e = np.histogram(f[:, j], bins=50)
                    c1.append(h)
                    edges.append(e)
                for i in range(6):
                    for j in range(i):
                        c2.append(numpy_counts2d(f[:, j], f[:, i], edges[j], edges[i]))
            return np.array(c1).reshape(k, 6, 50), np.array(c2).reshape(k, 15, 50, 50)

        parts = [
            ('quantiles', lambda: summary.quantiles(ser, n, Q), host_quantiles, lambda d, h: np.array_equal(d, h),
             SEL_PASSES * 6),
            ('marginals', lambda: summary.marginals(ser, n, mcols, 75, 'reference')[1], host_marginals,
             lambda d, h: np.array_equal(d, h), (SEL_PASSES + 1) * 6),                # (the ratio column reads two)
            ('corner_counts', lambda: summary.corner_counts(ser, n, list(range(6)), 50), host_corner,
             lambda d, h: np.array_equal(d[1], h[0]) and np.array_equal(d[3], h[1]), (SEL_PASSES + 1) * 6 + 2 * 15),
        ]
        for name, dev_fn, host_fn, same, col_reads in parts:
            dev_fn()   # (warm-up: scratch tables are sized on first use)
            dev_ms, dev = timed(dev_fn, a.reps)
            host_ms, host = timed(host_fn, host_reps)
            out({'what': name, 'members': k, 'walkers': nw, 'rows': n, 'ndim': 6, 'values_per_column': total,
                 'device_ms': float(np.median(dev_ms)), 'host_ms': float(np.min(host_ms)),
                 'speedup': float(np.min(host_ms) / np.median(dev_ms)), 'exact': bool(same(dev, host)),
                 'stream_bytes': int(col_reads * total * 8), 'device_ms_all': dev_ms, 'host_ms_all': host_ms})
        ser.close()
        del x, flats
    if a.out:
        with open(a.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
