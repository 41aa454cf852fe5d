#!/usr/bin/env python3
"""The pre-optimiser's host loop (optimizer.fit_spec_batch) against the device-resident run (optimizer.fit_spec_device;
DESIGN.md section 13) in one process, same start points and same draws, as JSON lines (and into --out):
  * config2: bench.py's flagship problem (4096 px, contrast terms) at the reference's optimiser shape -- 150 start
    points, nstep 400 (param_koi2298.txt:50-51), start points drawn as optimize_fit draws them;
  * koi: the first KOI target of bench.py's config 5 (2,064-2,349 px), same shape.
Per shape: --reps alternating blocks after one warm-up of each side; medians of the blocks' wall times, the trips
(host: launches of msx_opt_step; resident: draws of the longest chain), the evaluated trips (proposals that reached the
kernel, the same on both sides), microseconds per trip, the ratio host / resident, and where the resident run's wall time
goes (start points' chi^2 and upload; draw, queue and collect; rebuilding the chains in Python)."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def draw_starts(rng, nwalk, tmin, tmax, dist_arr):
    """optimize_fit's start points for a binary (mft6.py:1712-1743)."""
    t1 = rng.uniform(tmin, tmax, nwalk)
    t2 = np.array([rng.uniform(tmin, tt) for tt in t1])
    e1 = rng.uniform(0.1, 0.5, nwalk)
    rg1 = rng.uniform(0.05, 1, nwalk)
    rg2 = np.array([rng.uniform(0.05, r) / r for r in rg1])
    dist = np.abs(rng.normal(dist_arr[0], dist_arr[1], nwalk))
    return np.column_stack([t1, t2, e1, rg1, rg2, dist])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--starts', type=int, default=150)
    ap.add_argument('--steps', type=int, default=400)
    ap.add_argument('--reps', type=int, default=3)
    ap.add_argument('--chunk', type=int, default=128)
    ap.add_argument('--shapes', default='config2,koi')
    a = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process, see mcmc_spec_amd/_lib.py)
    import bench
    from mcmc_spec_amd import optimizer, synth
    from mcmc_spec_amd.engine import Engine
    lines = []

    def out(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    dist_prior = (2.0732e-3, 0.0277e-3)
    av_table = synth.make_av_table()
    matrix = synth.make_isochrone_matrix()
    grid = None
    for shape in a.shapes.split(','):
        eng = Engine(0)
        if shape == 'config2':
            W = bench.build_workload(eng, 4096, False, keep_host_grid=True)
            grid, tmin, tmax, npix = W['flux'], W['tmin'], W['tmax'], 4096
        else:
            info = bench.build_koi_problem(eng, 0, grid=grid)
            grid, tmin, tmax, npix = info['flux'], info['tmin'], info['tmax'], info['npix']
        starts = draw_starts(np.random.default_rng(4), a.starts, tmin, tmax, dist_prior)
        launches = [0]
        real = eng.ctx.opt_step

        def counted(*args, **kw):
            launches[0] += 1
            return real(*args, **kw)
        eng.ctx.opt_step = counted

        def run(fn, **kw):
            rngs = [np.random.default_rng(5000 + c) for c in range(a.starts)]
            launches[0] = 0
            t0 = time.perf_counter()
            res = fn(eng, starts, [tmin, tmax], dist_prior, matrix, av_table, nspec=2, steps=a.steps, dist_fit=True,
                     rad_prior=True, rngs=rngs, **kw)
            return time.perf_counter() - t0, res
        host_s, dev_s, dev_parts = [], [], []
        for rep in range(a.reps + 1):  # (block 0: warm-up of both sides)
            th, rh = run(optimizer.fit_spec_batch)
            rounds = launches[0]
            parts = {}
            td, rd = run(optimizer.fit_spec_device, chunk=a.chunk, timings=parts)
            if rep:
                host_s.append(th)
                dev_s.append(td)
                dev_parts.append(parts)
        evaluated = sum(len(ch.savetest) for _, _, ch in rh)
        assert evaluated == sum(len(ch.savetest) for _, _, ch in rd)
        same_rows = all(np.array_equal(np.concatenate([np.ravel(v) for v in x.gi]), np.concatenate([np.ravel(v) for v in y.gi]))
                        for (_, _, x), (_, _, y) in zip(rh, rd))
        trips = max(ch.trips for _, _, ch in rd)
        hm, dm = float(np.median(host_s)), float(np.median(dev_s))
        out({'what': 'opt_device', 'shape': shape, 'npix': int(npix), 'starts': a.starts, 'steps': a.steps, 'chunk': a.chunk,
             'host_wall_s': hm, 'resident_wall_s': dm, 'host_wall_s_all': host_s, 'resident_wall_s_all': dev_s,
             'host_trips': int(rounds), 'resident_trips': int(trips), 'evaluated_trips': int(evaluated),
             'host_us_per_trip': 1e6 * hm / rounds, 'resident_us_per_trip': 1e6 * dm / trips, 'host_over_resident': hm / dm,
             'resident_parts_s': {k: float(np.median([p[k] for p in dev_parts])) for k in ('init', 'run', 'rebuild')},
             'resident_run_us_per_trip': 1e6 * float(np.median([p['run'] for p in dev_parts])) / trips,
             'same_best_rows': bool(same_rows)})
        del eng
    if a.out:
        with open(a.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
