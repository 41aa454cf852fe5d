#!/usr/bin/env python3
"""Cost of component grids (DESIGN.md "Component grids") on the bench's 26 x 4 x 135,000 grid, as JSON lines (and into
the file named by --out):
  * staging: Gaussian + one rotation of the whole grid (v sin i 60, limb 0.6) against Gaussian + split into two copies +
    rotation of each copy ((60, 0.6) and (12, 0.3)), over config 2's and config 4's data windows (wall time of the
    synchronous calls, median of 5);
  * device memory per copy: the grid rows and the per-node tables staged for config 2's problem;
  * launch time (config 2, the automatic form): the 1-copy rotated grid against the 2-copy one, 256 and 2,048 walkers,
    three alternating rounds of 200 back-to-back launches timed by events."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def staging_ms(eng, wl, teffs, loggs, flux, win, vsini, limb, reps=5):
    ts = []
    for _ in range(reps):
        eng.stage_grid(wl, teffs, loggs, flux)
        t0 = time.perf_counter()
        eng.broaden_grid_window(win, 1700, vsini=vsini, limb=limb)   # every entry synchronises before it returns
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts))


def launch_us(eng, th, torch, reps=200):
    from mcmc_spec_amd import _lib
    d_th = torch.tensor(th, device='cuda')
    n, ndim = th.shape
    lp = torch.empty(n, dtype=torch.float64, device='cuda')
    st = torch.empty(n, dtype=torch.int32, device='cuda')
    s = torch.cuda.current_stream()

    def go():
        eng.ctx.logprob_batch_dev(d_th.data_ptr(), n, ndim, lp.data_ptr(), st.data_ptr(), s.cuda_stream, _lib.MODE_LOGPOST)
    for _ in range(20):
        go()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(s)
    for _ in range(reps):
        go()
    e1.record(s)
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e3 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process, see mcmc_spec_amd/_lib.py)
    from bench import build_workload
    from mcmc_spec_amd import synth
    from mcmc_spec_amd.engine import Engine
    wl = np.arange(3000, 30000, 0.2)
    teffs, loggs = np.arange(3000, 5600, 100), np.array([4.0, 4.5, 5.0, 5.5])
    flux = synth.make_grid(teffs, loggs, wl)
    rows = len(teffs) * len(loggs)
    lines = []

    def out(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    eng = Engine(0)
    for cfg, npix in (('config2', 4096), ('config4', 16384)):
        w = synth.data_wavelengths_um(npix)
        win = [np.floor(w.min() * 1e4), np.ceil(w.max() * 1e4)]
        n = int(np.sum((wl >= win[0]) & (wl <= win[1])))
        one = staging_ms(eng, wl, teffs, loggs, flux, win, 60.0, 0.6)
        two = staging_ms(eng, wl, teffs, loggs, flux, win, (60.0, 12.0), (0.6, 0.3))
        gauss = staging_ms(eng, wl, teffs, loggs, flux, win, 0, 0)
        out(dict(what='staging_ms', case=cfg, rows=rows, n=n, gaussian=gauss, gaussian_rotate_1copy=one,
                 gaussian_split_rotate_2copies=two))
    del eng

    # config 2: 1-copy rotated and 2-copy rotated grids, the same problem
    e1 = Engine(0)
    W = build_workload(e1, 4096, False, keep_host_grid=True, grid=flux)
    from mcmc_spec_amd import bands
    bl = bands.make_bands(W['tabs'], *W['vega'])
    kw = dict(nspec=2, bands=bl, av_table=synth.make_av_table(), tmin=W['tmin'], tmax=W['tmax'], prior=W['prior'])
    engs = {}
    for name, vs, ls in (('1copy', 60.0, 0.6), ('2copies', (60.0, 12.0), (0.6, 0.3))):
        e = Engine(0)
        e.stage_grid(W['wl'], W['teffs'], W['loggs'], W['flux'])
        e.broaden_grid_window(W['win'], W['resolution'], vsini=vs, limb=ls)
        e.stage_problem(W['data'], W['err'], W['fr'], W['r'], W['ctm'], W['ptm'], W['tmi'], W['tma'], W['matrix'], **kw)
        engs[name] = e
    npair = ((4096 + 511) // 512) * 256
    nquad = (npair + 1023) // 1024 * 512
    nb = len(W['fr'][2]) + len(W['fr'][5])
    per_row = 8 * len(wl) + 16 * npair + 8 * npair + 2 * 16 * nquad + 8 * nb
    out(dict(what='bytes_per_copy', case='config2', rows=rows, grid=rows * 8 * len(wl),
             tables=rows * (per_row - 8 * len(wl)), total=rows * per_row))
    for nw in (256, 2048):
        th = synth.draw_walkers(nw, seed=nw, tmin=W['tmin'], tmax=W['tmax'])
        res = {k: [] for k in engs}
        for _ in range(3):
            for k, e in engs.items():
                res[k].append(launch_us(e, th, torch))
        out(dict(what='launch_us', case='config2', walkers=nw, **res))
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(''.join(json.dumps(r) + '\n' for r in lines))


if __name__ == '__main__':
    main()
