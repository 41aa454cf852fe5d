#!/usr/bin/env python3
"""What a set of moves costs per iteration on the device-resident samplers, as JSON lines (and
into the file named by --out, default profiles/moves_bench.jsonl), at two shapes:
  * config2: one target, 256 walkers x 4,096 pixels (bench.py's flagship; the default run overlaps its half-steps there);
  * koi8x50: the eight KOI targets of tests/golden/golden_koi.npz, 50 walkers each, one target group.
Three variants alternate in one process after a warm-up round, every one with rng='device' (nothing is drawn on the host):
  * default: the run without moves= (the fused stretch kernel, one launch per half-step);
  * stretch_general: the stretch move forced through the path beside the kernel (step kernel, plain evaluation, step kernel);
  * mixture: [(StretchMove, .5), (DEMove, .4), (DEMove(gamma0=1), .1)].
The time is taken between the completions of two chunks of a run that keeps two chunks queued: from the return of the
collect call that ends the first `--skip` iterations to the return of the run's last collect, over the iterations between
them (>= 2,000) -- the GPU never idles in that interval, and begin / end (allocations, the state's upload) fall outside it.
(The library's streams are its own: no event of the caller's can be recorded on them.)  Medians over `--rounds` rounds,
every round's value, the variants' acceptance fractions, and the differences to the default run per half-step."""
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

VARIANTS = ('default', 'stretch_general', 'mixture')


def variant_kw(name):
    from mcmc_spec_amd.moves import DEMove, StretchMove
    if name == 'default':
        return {}
    if name == 'stretch_general':
        return dict(moves=StretchMove(2.0), _general=True)
    return dict(moves=[(StretchMove(), 0.5), (DEMove(), 0.4), (DEMove(gamma0=1.0), 0.1)])


def timed(owner, run, skip):
    """run() with owner.sampler_collect wrapped: us per iteration between the collect that completes `skip` iterations and the last."""
    marks, done = [], [0]
    inner = owner.sampler_collect

    def collect(slot, nsteps):
        out = inner(slot, nsteps)
        done[0] += nsteps
        marks.append((done[0], time.perf_counter()))
        return out
    owner.sampler_collect = collect
    try:
        run()
    finally:
        del owner.sampler_collect
    first = next(m for m in marks if m[0] >= skip)
    return (marks[-1][1] - first[1]) / (marks[-1][0] - first[0]) * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'moves_bench.jsonl'))
    ap.add_argument('--iters', type=int, default=2048, help='timed iterations per run')
    ap.add_argument('--skip', type=int, default=256, help='iterations of a run before the clock starts')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--chunk', type=int, default=64)
    a = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process, see mcmc_spec_amd/_lib.py)
    import bench
    from mcmc_spec_amd import synth
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler, State
    from group_profile import koi_engines
    lines = []
    total = a.skip + a.iters

    def measure(shape, make, owner, start, nwalkers):
        def run(name):
            s = make(**variant_kw(name))
            t = timed(owner, lambda: s.run_mcmc(start, total, store=False), a.skip)
            acc = s.acceptance_fraction
            return t, float(np.mean([np.mean(x) for x in acc]) if isinstance(acc, list) else np.mean(acc)), getattr(s, 'overlapped', None)
        rec = {'what': 'moves_us_per_iter', 'shape': shape, 'walkers': nwalkers, 'iters': a.iters, 'skip': a.skip, 'chunk': a.chunk}
        info = {}
        for name in VARIANTS:   # warm-up round
            try:
                info[name] = run(name)
            except (KeyError, IndexError, ValueError, RuntimeError) as e:   # (a walker error ends a run: recorded, not hidden)
                rec[name + '_error'] = '{}: {}'.format(type(e).__name__, e)
        names = [n for n in VARIANTS if n in info]
        rounds = {n: [] for n in names}
        for r in range(a.rounds):
            for n in names[r % len(names):] + names[:r % len(names)]:
                rounds[n].append(run(n)[0])
        for n in names:
            rec[n] = float(np.median(rounds[n]))
            rec[n + '_rounds'] = rounds[n]
            rec[n + '_acceptance'] = info[n][1]
            if info[n][2] is not None:
                rec[n + '_overlapped'] = info[n][2]
        if 'default' in rec:
            rec['default_spread'] = max(rounds['default']) - min(rounds['default'])
            for n in names[1:]:
                rec[n + '_minus_default_us_per_half_step'] = (rec[n] - rec['default']) / 2.0
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    eng = Engine(0)
    W = bench.build_workload(eng, 4096, False)
    p0 = synth.draw_walkers(256, seed=5, tmin=W['tmin'], tmax=W['tmax'])
    start = State(p0, eng.logposterior(p0))
    measure('config2', lambda **kw: DeviceEnsembleSampler(256, 6, eng, seed=17, chunk=a.chunk, rng='device', **kw), eng.ctx, start, 256)
    # ... and the default run with plain launches: what the path beside the kernel is one launch per half-step away from
    try:
        s = DeviceEnsembleSampler(256, 6, eng, seed=17, chunk=a.chunk, rng='device', overlap=False)
        lines[-1]['default_plain_launches'] = timed(eng.ctx, lambda: s.run_mcmc(start, total, store=False), a.skip)
        print(json.dumps({'what': 'default_plain_launches', 'shape': 'config2', 'us_per_iter': lines[-1]['default_plain_launches']}), flush=True)
    except (KeyError, IndexError, ValueError, RuntimeError) as e:
        lines[-1]['default_plain_launches_error'] = str(e)

    c, engines = koi_engines()
    grp = TargetGroup(engines[:8])
    p0s = [synth.draw_walkers(50, seed=60 + k, tmin=c.tmin, tmax=c.tmax) for k in range(8)]
    starts = [State(p, lp) for p, lp in zip(p0s, grp.logposterior(p0s))]
    measure('koi8x50', lambda **kw: DeviceGroupSampler([50] * 8, 6, grp, seeds=[1000 + k for k in range(8)], chunk=a.chunk, rng='device', **kw),
            grp.group, starts, 400)
    grp.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
