#!/usr/bin/env python3
"""Device-resident chains over a target group on the eight KOI targets of
tests/golden/golden_koi.npz, as JSON lines (and into the file named by --out): wall time of `run_mcmc` per iteration for
K targets x n walkers, three drivers alternating in one process, medians of `rounds` rounds after a warm-up round:
  * device: DeviceGroupSampler (one group launch per half-step, the ensembles resident);
  * group_host: GroupSampler over TargetGroup.logposterior (one synchronous group launch per half-step);
  * solo_device: the K targets' own DeviceEnsembleSamplers, run one after another.
The warm-up round checks the values first: every driver's chain of every target is the same, bit for bit."""
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

CONFIGS = [(8, 50), (8, 16), (8, 512), (1, 50), (2, 50)]
DRIVERS = ('device', 'group_host', 'solo_device')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--iters', type=int, default=300)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--configs', default=None, help='e.g. 8x50,2x50 (default: all five)')
    ap.add_argument('--drivers', default=','.join(DRIVERS))
    a = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process, see mcmc_spec_amd/_lib.py)
    from mcmc_spec_amd import synth
    from mcmc_spec_amd.group import DeviceGroupSampler, GroupSampler, TargetGroup
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    from group_profile import koi_engines
    c, engines = koi_engines()
    configs = CONFIGS if not a.configs else [tuple(int(v) for v in s.split('x')) for s in a.configs.split(',')]
    drivers = a.drivers.split(',')
    lines = []

    def out(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    for K, nw in configs:
        members = engines[:K]
        grp = TargetGroup(members)
        seeds = [1000 + k for k in range(K)]
        p0s = [synth.draw_walkers(nw, seed=60 + k, tmin=c.tmin, tmax=c.tmax) for k in range(K)]
        lp0 = grp.logposterior(p0s)
        from mcmc_spec_amd.sampler import State
        starts = [State(p, lp) for p, lp in zip(p0s, lp0)]

        def run(driver):
            t0 = time.perf_counter()
            if driver == 'device':
                s = DeviceGroupSampler([nw] * K, 6, grp, seeds=seeds, chunk=a.chunk)
                s.run_mcmc(starts, a.iters)
                chains = [s.get_chain(k) for k in range(K)]
            elif driver == 'group_host':
                s = GroupSampler([nw] * K, 6, grp.logposterior, seeds=seeds)
                s.run_mcmc(starts, a.iters)
                chains = [s.get_chain(k) for k in range(K)]
            else:
                chains = []
                for k, eng in enumerate(members):
                    s = DeviceEnsembleSampler(nw, 6, eng, seed=seeds[k], chunk=a.chunk)
                    s.run_mcmc(starts[k], a.iters)
                    chains.append(s.get_chain())
            return (time.perf_counter() - t0) / a.iters * 1e6, chains

        ref = None
        for d in drivers:  # warm-up round: values first
            _, ch = run(d)
            if ref is None:
                ref = ch
            assert all(np.array_equal(x, y) for x, y in zip(ch, ref)), (K, nw, d)
        rounds = {d: [] for d in drivers}
        for _ in range(a.rounds):
            for d in drivers:
                rounds[d].append(run(d)[0])
        rec = {'what': 'chain_us_per_iter', 'targets': K, 'walkers_per_target': nw, 'iters': a.iters, 'chunk': a.chunk}
        for d in drivers:
            rec[d] = float(np.median(rounds[d]))
        for d in drivers:
            rec[d + '_rounds'] = rounds[d]
        if 'device' in rec and 'group_host' in rec:
            rec['device_over_group_host'] = rec['device'] / rec['group_host']
        if 'device' in rec and 'solo_device' in rec:
            rec['device_over_solo_device'] = rec['device'] / rec['solo_device']
        rec['kernel'] = grp.launch_info([nw // 2] * K)['kernel']
        out(rec)
        grp.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
