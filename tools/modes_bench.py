#!/usr/bin/env python3
"""What the mixture fit of the posterior's modes costs on a resident series, as JSON lines (and into
--out, default profiles/modes_bench.jsonl), in one process on one GPU.  Two shapes -- one chain of 50 walkers x 15,000 rows x
6 columns, and 8 members of 50 walkers each -- drawn from a 0.8 / 0.2 mixture in the fit's units whose modes overlap in every
single column (so that the starts need their iterations), with ncomp = 2, six starts and max_iter = 50:
  * device: ``modes.fit_device`` (msx_series_moments, the thresholds' order statistics, msx_series_modes), a host clock around
    the synchronous calls; the median of --reps calls after a warm-up; msx_series_modes alone likewise, and the labels + split
    call (msx_series_mode_labels with per-mode series);
  * host: ``modes.fit`` on the same array in the same process, the best of 3 runs (without the download a resident chain
    would need first, which is timed on its own).  ``--host-members N`` times the first N members only and scales.
The two results are compared start by start (1e-9 relative; covariances relative to the standard deviations).  The launches
of the fit call: 2 (max_iter + 1)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, NDIM, NW = 15000, 6, 50
SHAPES = (('1 x 50', 1), ('8 x 50', 8))
CENTER = np.array([3850.0, 3400.0, 0.30, 0.45, 0.80, 2.0e-3])
WIDTH = np.array([100.0, 80.0, 0.05, 0.02, 0.04, 2.0e-5])


def clock(fn):
    t0 = time.perf_counter()
    res = fn()
    return 1e3 * (time.perf_counter() - t0), res


def draw(rows, nw, seed):
    """Two modes 2 sigma apart in each of three columns (3.5 sigma jointly), the light one narrower."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(rows, nw, NDIM))
    light = rng.random((rows, nw)) < 0.2
    x[light] = 0.6 * x[light] + np.array([2.0, -2.0, 0.0, 2.0, 0.0, 0.0])
    return CENTER + WIDTH * x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'modes_bench.jsonl'))
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--rows', type=int, default=ROWS)
    ap.add_argument('--max-iter', type=int, default=50)
    ap.add_argument('--host-runs', type=int, default=3, help='runs of modes.fit, the best of which counts')
    ap.add_argument('--host-members', type=int, default=0,
                    help='time modes.fit on the first N members only and scale to all of them (0: all; the members are fitted one '
                         'after the other and have one shape)')
    a = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process, see mcmc_spec_amd/_lib.py)
    from mcmc_spec_amd import _lib, modes
    from mcmc_spec_amd.engine import Engine
    ctx = Engine(0).ctx
    lines = []
    for name, k in SHAPES:
        counts = [NW] * k
        chain = draw(a.rows, NW * k, k)
        ser = _lib.Series(ctx, NW * k, NDIM, counts, cap_hint=a.rows)
        ser.append(chain)
        kw = dict(ncomp=2, max_iter=a.max_iter)
        fit = lambda: modes.fit_device(ser, a.rows, ctx=ctx, **kw)
        dev = fit()   # warm-up: code objects, the scratch buffer
        em = lambda: ser.modes(a.rows, 0, 1, dev.cols, dev.center, dev.scale, 2, dev.split_col, dev.split_at, a.max_iter)

        def split():
            parts = dev.split()
            for row in parts:
                for s in row:
                    s.close()
        em(), split()
        full_niter = dev.niter
        t_fit = [clock(fit)[0] for _ in range(a.reps)]
        t_em = [clock(em)[0] for _ in range(a.reps)]
        t_split = [clock(split)[0] for _ in range(a.reps)]
        t_read = [clock(lambda: ser.read(0, a.rows))[0] for _ in range(3)]
        t_host, ref = [], None
        hm = k if a.host_members < 1 else min(a.host_members, k)
        for _ in range(a.host_runs):
            t, ref = clock(lambda: modes.fit(chain[:, :NW * hm], counts[:hm], **kw))
            t_host.append(t * k / hm)
        dev = dev.select(list(range(hm)))
        sd = np.sqrt(np.diagonal(ref.cov, axis1=-2, axis2=-1))
        rel = {'weight': np.max(np.abs(dev.weight - ref.weight) / ref.weight), 'loglik': np.max(np.abs(dev.loglik - ref.loglik) / np.abs(ref.loglik)),
               'mean': np.max(np.abs(dev.mean - ref.mean) / np.abs(ref.mean)),
               'cov': np.max(np.abs(dev.cov - ref.cov) / (sd[..., :, None] * sd[..., None, :]))}
        agree = bool(max(rel.values()) <= 1e-9 and np.array_equal(dev.niter, ref.niter) and np.array_equal(dev.status, ref.status))
        iters = int(np.sum(ref.niter))
        # bytes the statistics kernels read: every iteration of every start and component reads the member's d columns
        streamed = 8.0 * a.rows * NW * NDIM * 2 * float(np.sum(full_niter + 1))
        rec = {'what': 'modes_fit', 'shape': name, 'members': k, 'walkers': NW * k, 'rows': a.rows, 'ndim': NDIM, 'ncomp': 2, 'nstarts': NDIM,
               'max_iter': a.max_iter, 'reps': a.reps, 'launches': 2 * (a.max_iter + 1), 'device_fit_ms': float(np.median(t_fit)),
               'device_em_ms': float(np.median(t_em)), 'device_labels_split_ms': float(np.median(t_split)),
               'download_ms': float(np.median(t_read)), 'host_ms': float(np.min(t_host)), 'speedup': float(np.min(t_host) / np.median(t_fit)),
               'em_ms_per_launch_pair': float(np.median(t_em) / (a.max_iter + 1)), 'em_gb_per_s': streamed / (np.median(t_em) * 1e-3) / 1e9,
               'iterations_run': iters, 'niter': ref.niter.tolist(), 'status': ref.status.tolist(), 'agree': agree,
               'worst_rel': {n: float(v) for n, v in rel.items()}, 'host_members_timed': hm, 'host_runs': a.host_runs, 'heavy_weight': dev.weight[np.arange(hm), dev.best, 0].tolist(),
               'device_fit_all_ms': t_fit, 'host_all_ms': t_host}
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
