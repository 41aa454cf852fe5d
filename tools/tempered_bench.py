#!/usr/bin/env python3
"""What a tempered iteration costs on the device-resident sampler, as JSON lines (and into the file
named by --out, default profiles/tempered_bench.jsonl), on config 2's problem (bench.py's flagship: 4,096 pixels):
  * general_256: ONE chain of 256 walkers through the path beside the fused kernel as the parent commit has it
    (DeviceEnsembleSampler(moves=StretchMove(), _general=True): msx_sampler_enqueue_moves_drawn, code this change does not
    touch) -- the yardstick: T untied chains cost T times this today;
  * T1_256, T4_256, T8_256: ladders of 1, 4 and 8 rungs of 256 walkers;
  * T8_512: 8 rungs of 512 walkers -- 2,048 proposals per launch, where MSX_PATH_AUTO takes the pair form.
Every variant with rng='device' (nothing is drawn on the host) and the stretch move.  tools/moves_bench.py's method: the
time is taken between the completions of two chunks of a run that keeps two chunks queued -- from the return of the collect
call that ends the first `--skip` iterations to the return of the run's last collect -- so the GPU never idles in the
interval and begin / end fall outside it.  The variants alternate in one process after a warm-up round; medians over
`--rounds` rounds, every round's value, msx_last_form after each variant's run, the ladders' swap and acceptance
fractions, and each ladder against T times the yardstick.

--adaptive (into profiles/tempered_adaptive_bench.jsonl): what the adaptive ladder adds to an iteration,
at T = 4 x 256 and T = 8 x 256, by the same method.  The driver holds no GPU: it starts `--processes` pairs of fresh child
processes in alternating order -- one on THIS tree, timing the fixed and the adaptive ladder in alternating rounds after a
warm-up round; one on the tree named by --parent-tree (a built checkout of the parent commit), timing its fixed ladder, the
yardstick -- and reports medians, every value, the spreads, adaptive minus fixed, and this tree's fixed ladder minus the
parent's.  The child of this tree also reports the swap fractions of default_betas(8, beta_min) before and after
`--adapt-iters` adaptive iterations (adaptation_lag 1000, adaptation_time 10), the latter from a frozen run."""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROOT = HERE
if '--tree' in sys.argv:   # (a child of --adaptive: import the package and bench.py of that tree)
    ROOT = os.path.abspath(sys.argv[sys.argv.index('--tree') + 1])
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

LADDERS = (('T1_256', 1, 256), ('T4_256', 4, 256), ('T8_256', 8, 256), ('T8_512', 8, 512))
FORMS = {0: 'fused', 1: 'pair', 2: 'linked', 3: 'inpath'}


def timed(owner, attr, run, skip):
    """run() with owner.<attr> (a collect call) wrapped: us per iteration between the collect that completes `skip`
    iterations and the last."""
    marks, done = [], [0]
    inner = getattr(owner, attr)

    def collect(slot, nsteps):
        out = inner(slot, nsteps)
        done[0] += nsteps
        marks.append((done[0], time.perf_counter()))
        return out
    setattr(owner, attr, collect)
    try:
        run()
    finally:
        delattr(owner, attr)
    first = next(m for m in marks if m[0] >= skip)
    return (marks[-1][1] - first[1]) / (marks[-1][0] - first[0]) * 1e6


ADAPTIVE_LADDERS = (('T4_256', 4, 256), ('T8_256', 8, 256))


def adaptive_child(a):
    """One process of --adaptive on the tree ROOT: JSON lines {variant, rounds, ...} on stdout."""
    import torch  # noqa: F401
    import bench
    from mcmc_spec_amd import synth
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd.tempered import DeviceTemperedSampler, TemperedState, default_betas
    total = a.skip + a.iters
    eng = Engine(0)
    W = bench.build_workload(eng, 4096, False)
    ctx = eng.ctx
    starts = {}
    for name, T, nw in ADAPTIVE_LADDERS:
        p = synth.draw_walkers(T * nw, seed=5 + T * nw, tmin=W['tmin'], tmax=W['tmax'])
        starts[name] = TemperedState(p.reshape(T, nw, 6), eng.loglikelihood(p).reshape(T, nw), eng.logprior(p).reshape(T, nw))
    kinds = ('fixed',) if a.tree else ('fixed', 'adaptive')

    def run(name, kind):
        T, nw = next((T, nw) for n, T, nw in ADAPTIVE_LADDERS if n == name)
        kw = dict(adaptive=True) if kind == 'adaptive' else {}   # (the defaults: lag 10,000, time 100 -- the cost does not depend on them)
        s = DeviceTemperedSampler(nw, 6, eng, betas=default_betas(T, a.beta_min), seed=17, chunk=a.chunk, rng='device', **kw)
        t = timed(ctx, 'tempered_collect', lambda: s.run_mcmc(starts[name], total, store=False), a.skip)
        return t, {'swap_fraction': [float(x) for x in s.swap_fraction], 'ntemps': T, 'walkers_per_rung': nw}

    names = [(n, k) for n, _, _ in ADAPTIVE_LADDERS for k in kinds]
    info = {v: run(*v)[1] for v in names}   # warm-up round
    rounds = {v: [] for v in names}
    for r in range(a.rounds):
        for v in names[r % len(names):] + names[:r % len(names)]:
            rounds[v].append(run(*v)[0])
    for v in names:
        rec = {'variant': v[0] + '_' + v[1], 'tree': 'parent' if a.tree else 'this', 'rounds': rounds[v]}
        rec.update(info[v])
        print('CHILD ' + json.dumps(rec), flush=True)
    if not a.tree and a.adapt_iters > 0:
        s = DeviceTemperedSampler(256, 6, eng, betas=default_betas(8, a.beta_min), seed=17, chunk=a.chunk, rng='device', adaptive=True,
                                  adaptation_lag=1000.0, adaptation_time=10.0)
        before = [float(x) for x in s.betas]
        st = s.run_mcmc(starts['T8_256'], a.adapt_iters, store=False)
        during = [float(x) for x in s.swap_fraction]
        s.reset()
        s.run_mcmc(st, a.iters, store=False, adapt=False)
        print('CHILD ' + json.dumps({'variant': 'T8_256_ladder', 'tree': 'this', 'adapt_iters': a.adapt_iters, 'frozen_iters': a.iters,
                                     'betas_before': before, 'betas_after': [float(x) for x in s.betas], 'skipped': s.ladder_skipped,
                                     'swap_fraction_fixed': info[('T8_256', 'fixed')]['swap_fraction'], 'swap_fraction_adapting': during,
                                     'swap_fraction_frozen': [float(x) for x in s.swap_fraction]}), flush=True)


def adaptive_driver(a):
    import subprocess
    trees = [None] + ([os.path.abspath(a.parent_tree)] if a.parent_tree else [])
    got, ladder = {}, None
    for i in range(a.processes):
        for tree in (trees if i % 2 == 0 else trees[::-1]):
            cmd = [sys.executable, os.path.abspath(__file__), '--adaptive-child', '--iters', str(a.iters), '--skip', str(a.skip), '--rounds',
                   str(a.rounds), '--chunk', str(a.chunk), '--beta-min', str(a.beta_min), '--adapt-iters', str(a.adapt_iters if i == 0 else 0)]
            out = subprocess.run(cmd + (['--tree', tree] if tree else []), stdout=subprocess.PIPE, text=True, check=True, cwd=tree or HERE).stdout
            for ln in out.splitlines():
                if not ln.startswith('CHILD '):
                    continue
                rec = json.loads(ln[6:])
                if rec['variant'].endswith('_ladder'):
                    ladder = rec
                    continue
                slot = got.setdefault((rec['variant'], rec['tree']), dict(rec, rounds=[]))
                slot['rounds'] += rec['rounds']
    lines = []
    for (variant, tree), rec in sorted(got.items()):
        rec.update({'what': 'tempered_adaptive_us_per_iter', 'shape': 'config2', 'iters': a.iters, 'skip': a.skip, 'chunk': a.chunk,
                    'us_per_iter': float(np.median(rec['rounds'])), 'spread': max(rec['rounds']) - min(rec['rounds'])})
        lines.append(rec)
    med = {(r['variant'], r['tree']): r['us_per_iter'] for r in lines}
    for name, _, _ in ADAPTIVE_LADDERS:
        rec = {'what': 'tempered_adaptive_difference', 'ladder': name,
               'adaptive_minus_fixed_us': med[(name + '_adaptive', 'this')] - med[(name + '_fixed', 'this')]}
        if (name + '_fixed', 'parent') in med:
            rec['fixed_minus_parent_fixed_us'] = med[(name + '_fixed', 'this')] - med[(name + '_fixed', 'parent')]
        lines.append(rec)
    if ladder is not None:
        lines.append(dict(ladder, what='tempered_adaptive_ladder', shape='config2'))
    for rec in lines:
        print(json.dumps(rec), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None, help='default profiles/tempered_bench.jsonl (--adaptive: profiles/tempered_adaptive_bench.jsonl)')
    ap.add_argument('--adaptive', action='store_true', help='the cost of the adaptive ladder (see above)')
    ap.add_argument('--parent-tree', default=None, help='--adaptive: a built checkout of the parent commit, for the yardstick')
    ap.add_argument('--processes', type=int, default=2, help='--adaptive: pairs of child processes')
    ap.add_argument('--adapt-iters', type=int, default=2000, help='--adaptive: adaptive iterations before the frozen run')
    ap.add_argument('--adaptive-child', action='store_true', help=argparse.SUPPRESS)
    ap.add_argument('--tree', default=None, help=argparse.SUPPRESS)
    ap.add_argument('--iters', type=int, default=2048, help='timed iterations per run')
    ap.add_argument('--skip', type=int, default=256, help='iterations of a run before the clock starts')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--beta-min', type=float, default=0.02)
    a = ap.parse_args()
    if a.adaptive_child:
        return adaptive_child(a)
    if a.out is None:
        a.out = os.path.join(HERE, 'profiles', 'tempered_adaptive_bench.jsonl' if a.adaptive else 'tempered_bench.jsonl')
    if a.adaptive:
        return adaptive_driver(a)
    import torch  # noqa: F401  (first: one HIP runtime per process, see mcmc_spec_amd/_lib.py)
    import bench
    from mcmc_spec_amd import synth
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd.moves import StretchMove
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler, State
    from mcmc_spec_amd.tempered import DeviceTemperedSampler, TemperedState, default_betas
    total = a.skip + a.iters
    eng = Engine(0)
    W = bench.build_workload(eng, 4096, False)
    ctx = eng.ctx

    p256 = synth.draw_walkers(256, seed=5, tmin=W['tmin'], tmax=W['tmax'])
    start256 = State(p256, eng.logposterior(p256))
    starts = {}
    for name, T, nw in LADDERS:
        p = synth.draw_walkers(T * nw, seed=5 + T * nw, tmin=W['tmin'], tmax=W['tmax'])
        starts[name] = TemperedState(p.reshape(T, nw, 6), eng.loglikelihood(p).reshape(T, nw), eng.logprior(p).reshape(T, nw))

    def run(name):
        if name == 'general_256':
            s = DeviceEnsembleSampler(256, 6, eng, seed=17, chunk=a.chunk, rng='device', moves=StretchMove(2.0), _general=True)
            t = timed(ctx, 'sampler_collect', lambda: s.run_mcmc(start256, total, store=False), a.skip)
            return t, {'acceptance': float(np.mean(s.acceptance_fraction)), 'form': FORMS[ctx.last_form()]}
        T, nw = next((T, nw) for n, T, nw in LADDERS if n == name)
        betas = default_betas(T, a.beta_min) if T > 1 else [1.0]
        s = DeviceTemperedSampler(nw, 6, eng, betas=betas, seed=17, chunk=a.chunk, rng='device')
        t = timed(ctx, 'tempered_collect', lambda: s.run_mcmc(starts[name], total, store=False), a.skip)
        return t, {'acceptance': [float(x) for x in s.acceptance_fraction.mean(axis=1)], 'swap_fraction': [float(x) for x in s.swap_fraction],
                   'form': FORMS[ctx.last_form()], 'ntemps': T, 'walkers_per_rung': nw, 'proposals_per_launch': T * nw // 2}

    names = ['general_256'] + [n for n, _, _ in LADDERS]
    info = {n: run(n)[1] for n in names}   # warm-up round
    rounds = {n: [] for n in names}
    for r in range(a.rounds):
        for n in names[r % len(names):] + names[:r % len(names)]:
            rounds[n].append(run(n)[0])
    base = float(np.median(rounds['general_256']))
    lines = []
    for n in names:
        rec = {'what': 'tempered_us_per_iter', 'variant': n, 'shape': 'config2', 'iters': a.iters, 'skip': a.skip, 'chunk': a.chunk,
               'us_per_iter': float(np.median(rounds[n])), 'rounds': rounds[n], 'spread': max(rounds[n]) - min(rounds[n])}
        rec.update(info[n])
        if n != 'general_256':
            T, nw = rec['ntemps'], rec['walkers_per_rung']
            rec['untied_chains_us'] = T * (nw // 256) * base          # T (x 2 at 512 walkers) chains of 256 through the parent's path
            rec['ratio_to_untied'] = rec['us_per_iter'] / rec['untied_chains_us']
            rec['evaluations_per_second'] = 2.0 * T * nw / (rec['us_per_iter'] * 1e-6)   # prior and likelihood of every proposal
        print(json.dumps(rec), flush=True)
        lines.append(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
