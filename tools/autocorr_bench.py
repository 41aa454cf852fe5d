#!/usr/bin/env python3
"""Autocorrelation time on the host and on the device, as JSON lines (and into --out), in one
process:
  * tau: one get_autocorr_time of synthetic AR(1) rows (rho 0.9, ndim 6) at 50 x 15,000, 256 x 5,000 and 1,024 x 15,000
    walkers x rows -- the host method (EnsembleSampler) against the device's (rows fed through msx_series_append),
    medians of --reps calls, with the lag tiles the device's window search took;
  * protocol: run_reference_protocol at the reference's shape (50 walkers of golden case A, --burn burn-in and --steps
    production iterations) with autocorr='host' and 'device' at nthin 100 and 10, next to a chain-only run of the same
    length;
  * group_protocol: run_group_protocol on the eight KOI targets x 50 walkers (DeviceGroupSampler, autocorr 'device'),
    next to a chain-only run of the same length."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SHAPES = [(50, 15000), (256, 5000), (1024, 15000)]


def ar1_rows(n, nw, ndim, rho, seed):
    rng = np.random.default_rng(seed)
    x = np.empty((n, nw, ndim))
    x[0] = rng.normal(size=(nw, ndim))
    s = np.sqrt(1.0 - rho * rho)
    for t in range(1, n):
        x[t] = rho * x[t - 1] + s * rng.standard_normal((nw, ndim))
    return x


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=5)
    ap.add_argument('--burn', type=int, default=200)
    ap.add_argument('--steps', type=int, default=3000)
    ap.add_argument('--parts', default='tau,protocol,group_protocol')
    a = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process, see mcmc_spec_amd/_lib.py)
    from mcmc_spec_amd import _lib, synth
    from mcmc_spec_amd.sampler import (ACF_TILE, DeviceEnsembleSampler, EnsembleSampler, _device_integrated_time,
                                       run_reference_protocol)
    from common import golden_case
    from test_gpu_parity import make_engine
    parts = a.parts.split(',')
    lines = []

    def out(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    c = golden_case('A')
    eng = make_engine(c)
    if 'tau' in parts:
        for nw, n in SHAPES:
            x = ar1_rows(n, nw, 6, 0.9, seed=nw + n)
            host = EnsembleSampler(nw, 6, None, vectorize=True, seed=0)
            host._chain = list(x)
            ser = _lib.Series(eng.ctx, nw, 6, cap_hint=n)
            ser.append(x)
            calls = []
            real = ser.acf

            def counted(*args, **kw):
                calls.append(args[3:5])
                return real(*args, **kw)
            ser.acf = counted
            _device_integrated_time(ser, n, 5.0, 0, 1)   # (warm-up)
            dev_ms, host_ms = [], []
            for _ in range(a.reps):
                calls.clear()
                t0 = time.perf_counter()
                td = _device_integrated_time(ser, n, 5.0, 0, 1)[0]
                dev_ms.append(1e3 * (time.perf_counter() - t0))
            for _ in range(max(1, min(a.reps, 3 if nw * n < 2e6 else 1))):
                t0 = time.perf_counter()
                th = host.get_autocorr_time(quiet=True)
                host_ms.append(1e3 * (time.perf_counter() - t0))
            out({'what': 'tau', 'walkers': nw, 'rows': n, 'ndim': 6, 'rho': 0.9, 'host_ms': float(np.median(host_ms)),
                 'device_ms': float(np.median(dev_ms)), 'speedup': float(np.median(host_ms) / np.median(dev_ms)),
                 'device_ms_all': dev_ms, 'host_ms_all': host_ms, 'tiles': [list(map(int, t)) for t in calls],
                 'max_rel_tau_diff': float(np.max(np.abs(td / th - 1)))})
            ser.close()
            del x, host

    if 'protocol' in parts:
        p0 = synth.draw_walkers(50, seed=9, tmin=c.tmin, tmax=c.tmax)
        s = DeviceEnsembleSampler(50, 6, eng, seed=1, chunk=64)
        t0 = time.perf_counter()
        st = s.run_mcmc(p0, a.burn)
        s.reset()
        s.run_mcmc(st, a.steps)
        chain_s = time.perf_counter() - t0
        out({'what': 'chain_only', 'walkers': 50, 'burn': a.burn, 'steps': a.steps, 'wall_s': chain_s})
        for nthin in (100, 10):
            res = {}
            for mode in ('host', 'device'):
                s = DeviceEnsembleSampler(50, 6, eng, seed=1, chunk=64, autocorr=mode)
                t0 = time.perf_counter()
                smp = run_reference_protocol(s, p0.copy(), a.burn, a.steps, nthin=nthin)
                res[mode] = (time.perf_counter() - t0, len(smp) // 50, smp)
            out({'what': 'protocol', 'walkers': 50, 'burn': a.burn, 'steps': a.steps, 'nthin': nthin,
                 'host_wall_s': res['host'][0], 'device_wall_s': res['device'][0], 'chain_only_wall_s': chain_s,
                 'stopped_at': {'host': res['host'][1], 'device': res['device'][1]},
                 'same_samples': bool(np.array_equal(res['host'][2], res['device'][2]))})

    if 'group_protocol' in parts:
        from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup, run_group_protocol
        from group_profile import koi_engines
        kc, engines = koi_engines()
        grp = TargetGroup(engines[:8])
        p0s = [synth.draw_walkers(50, seed=60 + k, tmin=kc.tmin, tmax=kc.tmax) for k in range(8)]
        seeds = [1000 + k for k in range(8)]
        dev = DeviceGroupSampler([50] * 8, 6, grp, seeds=seeds, chunk=64)
        t0 = time.perf_counter()
        st = dev.run_mcmc(p0s, a.burn)
        dev.reset()
        dev.run_mcmc(st, a.steps)
        chain_s = time.perf_counter() - t0
        for nthin in (100, 10):
            dev = DeviceGroupSampler([50] * 8, 6, grp, seeds=seeds, chunk=64, autocorr='device')
            t0 = time.perf_counter()
            smp = run_group_protocol(dev, [p.copy() for p in p0s], a.burn, a.steps, nthin=nthin)
            out({'what': 'group_protocol', 'targets': 8, 'walkers_per_target': 50, 'burn': a.burn, 'steps': a.steps, 'nthin': nthin,
                 'device_wall_s': time.perf_counter() - t0, 'chain_only_wall_s': chain_s,
                 'stopped_at': [len(x) // 50 for x in smp]})
        grp.close()
    if a.out:
        with open(a.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
