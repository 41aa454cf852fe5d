#!/usr/bin/env python3
"""Device-resident chains over a target group on the eight KOI targets of
tests/golden/golden_koi.npz, as JSON lines (and into the file named by --out): wall time of `run_mcmc` per iteration for
K targets x n walkers, four drivers alternating in one process, medians of `rounds` rounds after a warm-up round:
  * device: DeviceGroupSampler (one group launch per half-step, the ensembles resident; the host draws every chunk);
  * device_rng: DeviceGroupSampler(rng='device') (the device draws every chunk itself: DESIGN.md section 11.2);
  * group_host: GroupSampler over TargetGroup.logposterior (one synchronous group launch per half-step);
  * solo_device: the K targets' own DeviceEnsembleSamplers, run one after another.
The warm-up round checks the values first: every host-drawn driver's chain of every target is the same, bit for bit, and
the device-drawn driver's is its host twin's (GroupSampler fed the device generator's stream: msx_sampler_draw).
The drivers' order rotates from round to round.  Each line also carries, for the two DeviceGroupSampler drivers, the host
thread's time by phase, measured here by wrapping the Group's calls for the run (the library is not instrumented): per
run the sampler's construction, begin, waiting for the chunks' host draws, enqueue, collect, the rest of run_mcmc (chain
rows, States, the pump), end and get_chain -- every round's values and their medians -- and per chunk the four phases
that repeat (median over the rounds, us).  And the no-regression
condition of section 11.2: the device-drawn median may not exceed the host-drawn one by more than the host-drawn driver's
own min-max spread."""
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
DRIVERS = ('device', 'device_rng', 'group_host', 'solo_device')
PHASES = ('construct', 'begin', 'draw_wait', 'enqueue', 'collect', 'states', 'end', 'get_chain')
PER_CHUNK = ('draw_wait', 'enqueue', 'collect', 'states')


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

        split = {}   # driver -> the last run's host seconds per phase and its chunks

        def timed_device_run(rng):
            """One DeviceGroupSampler run with the host thread's time attributed from outside the library: the Group's
            begin / enqueue / collect / end calls and the sampler's draw callables are wrapped for this run only."""
            g = grp.group
            ph = {p: 0.0 for p in PHASES}
            ph['chunks'] = 0
            clock = time.perf_counter
            last_end = [0.0]
            done = {'split': [], 'moves': []}
            t0 = clock()
            s = DeviceGroupSampler([nw] * K, 6, grp, seeds=seeds, chunk=a.chunk, rng=rng)
            ph['construct'] = clock() - t0

            def draw(name, f):
                def call(m):
                    r = f(m)
                    done[name].append(clock())   # (a worker thread of the pump)
                    return r
                return call

            def wrap(name, f, is_enqueue=False):
                def call(*args, **kw):
                    t = clock()
                    if is_enqueue:
                        i = ph['chunks']
                        ph['chunks'] += 1
                        if rng == 'host':   # blocked on chunk i's draws: from the last library call's return until they were done
                            ph['draw_wait'] += min(max(max(done['split'][i], done['moves'][i]) - last_end[0], 0.0), t - last_end[0])
                    try:
                        return f(*args, **kw)
                    finally:
                        last_end[0] = clock()
                        ph[name] += last_end[0] - t
                return call
            s._draw_split_all, s._draw_moves_all = draw('split', s._draw_split_all), draw('moves', s._draw_moves_all)
            names = {'sampler_begin': 'begin', 'sampler_enqueue': 'enqueue', 'sampler_enqueue_drawn': 'enqueue', 'sampler_collect': 'collect',
                     'sampler_end': 'end'}
            for attr, name in names.items():
                setattr(g, attr, wrap(name, getattr(g, attr), name == 'enqueue'))
            try:
                t0 = clock()
                s.run_mcmc(starts, a.iters)
                total = clock() - t0
            finally:
                for attr in names:
                    delattr(g, attr)
            # what is left of run_mcmc: chain rows, States, the pump's own code
            ph['states'] = total - sum(ph[p] for p in ('begin', 'draw_wait', 'enqueue', 'collect', 'end'))
            t0 = clock()
            chains = [s.get_chain(k) for k in range(K)]
            ph['get_chain'] = clock() - t0
            return ph, chains

        def run(driver):
            t0 = time.perf_counter()
            if driver in ('device', 'device_rng'):
                split[driver], chains = timed_device_run('device' if driver == 'device_rng' else 'host')
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

        def twin():   # the device-drawn chains, walked by the host loop
            s = GroupSampler([nw] * K, 6, grp.logposterior,
                             draws=[(lambda i, m, k=k: members[k].ctx.sampler_draw(seeds[k], 2.0, i, m, nw, 6)) for k in range(K)])
            s.run_mcmc(starts, a.iters)
            return [s.get_chain(k) for k in range(K)]

        ref = None
        for d in drivers:  # warm-up round: values first
            _, ch = run(d)
            if d == 'device_rng':
                want = twin()
            else:
                ref = ch if ref is None else ref
                want = ref
            assert all(np.array_equal(x, y) for x, y in zip(ch, want)), (K, nw, d)
        rounds = {d: [] for d in drivers}
        phases = {d: {p: [] for p in PHASES} for d in drivers if d in ('device', 'device_rng')}
        for r in range(a.rounds):
            for d in drivers[r % len(drivers):] + drivers[:r % len(drivers)]:   # (no driver always follows the same one)
                rounds[d].append(run(d)[0])
                if d in phases:
                    for p in PHASES:
                        phases[d][p].append(split[d][p] * 1e3)   # ms per run
        rec = {'what': 'chain_us_per_iter', 'targets': K, 'walkers_per_target': nw, 'iters': a.iters, 'chunk': a.chunk}
        for d in drivers:
            rec[d] = float(np.median(rounds[d]))
        for d in drivers:
            rec[d + '_rounds'] = rounds[d]
        for d in phases:
            rec[d + '_chunks'] = split[d]['chunks']
            rec[d + '_host_us_per_chunk'] = {p: float(np.median(phases[d][p])) * 1e3 / split[d]['chunks'] for p in PER_CHUNK}
            rec[d + '_host_ms_per_run'] = {p: float(np.median(v)) for p, v in phases[d].items()}
            rec[d + '_host_ms_per_run_rounds'] = phases[d]
        if 'device' in rec and 'device_rng' in rec:
            rec['device_rng_over_device'] = rec['device_rng'] / rec['device']
            rec['device_spread'] = max(rounds['device']) - min(rounds['device'])
            rec['no_regression'] = bool(rec['device_rng'] - rec['device'] <= rec['device_spread'])
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
