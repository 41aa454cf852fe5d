#!/usr/bin/env python3
"""What an iteration of every target's ladder costs in ONE run, as JSON lines (and into the file named
by --out, default profiles/group_tempered_bench.jsonl), on the KOI targets of tests/golden/golden_koi.npz:
  * group: DeviceGroupTemperedSampler -- K targets x T rungs in eight launches per iteration;
  * solo: the yardstick, code this change does not touch -- the K targets' own DeviceTemperedSamplers, each on its own
    context, run one after another, their us per iteration SUMMED.
Shapes: the 8 targets x 50 walkers at T = 4 and T = 8 (config 5's ensembles with a ladder each), 8 x 256 at T = 8, and one
target x 256 at T = 8 (the group path against the single-target path on the same ladder).  tools/tempered_bench.py's method:
rng='device', the stretch move, us per iteration between the completions of two chunks of a run that keeps two chunks queued
(from the collect that ends the first `--skip` iterations to the run's last collect), the two drivers alternating in one
process after a warm-up round that also checks target 0's chain of the group run against its solo run bit for bit; medians
over `--rounds` rounds, every round's value, the ratio group / solo, and target 0's swap and acceptance fractions.  The 8 x 50
shapes carry the acceptance: ratio <= 0.5 (section 11's bar for a group launch against sequential ones)."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
sys.path.insert(0, os.path.join(ROOT, 'tests'))

SHAPES = (('K8_T4_50', 8, 4, 50), ('K8_T8_50', 8, 8, 50), ('K8_T8_256', 8, 8, 256), ('K1_T8_256', 1, 8, 256))
GATED = ('K8_T4_50', 'K8_T8_50')
BAR = 0.5


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'group_tempered_bench.jsonl'))
    ap.add_argument('--iters', type=int, default=2048, help='timed iterations per run')
    ap.add_argument('--skip', type=int, default=256, help='iterations of a run before the clock starts')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--beta-min', type=float, default=0.02)
    ap.add_argument('--shapes', default=None, help='e.g. K8_T8_50,K1_T8_256 (default: all four)')
    a = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process, see mcmc_spec_amd/_lib.py)
    from group_profile import koi_engines
    from mcmc_spec_amd import _lib, synth
    from mcmc_spec_amd.group import TargetGroup
    from mcmc_spec_amd.tempered import DeviceGroupTemperedSampler, DeviceTemperedSampler, TemperedState, default_betas
    from tempered_bench import timed
    c, engines = koi_engines()
    total = a.skip + a.iters
    shapes = [s for s in SHAPES if a.shapes is None or s[0] in a.shapes.split(',')]
    lines = []

    def start(eng, T, nw, seed):
        """T x nw walkers inside the prior with a clean likelihood, as a TemperedState."""
        cand = synth.draw_walkers(4 * T * nw, seed=seed, tmin=c.tmin, tmax=c.tmax)
        (lpr, st), (ll, stl) = eng.ctx.logprob_batch(cand, _lib.MODE_LOGPRIOR), eng.ctx.logprob_batch(cand, _lib.MODE_LOGLIKE)
        ok = np.nonzero(np.isfinite(lpr) & (st == 0) & (stl == 0) & np.isfinite(ll))[0][:T * nw]
        if len(ok) < T * nw:
            raise RuntimeError('not enough starting walkers inside the prior')
        return TemperedState(cand[ok].reshape(T, nw, 6), ll[ok].reshape(T, nw), lpr[ok].reshape(T, nw))

    for name, K, T, nw in shapes:
        members = engines[:K]
        grp = TargetGroup(members)
        betas = default_betas(T, a.beta_min)
        seeds = [1000 + 100 * k for k in range(K)]
        starts = [start(e, T, nw, 60 + k) for k, e in enumerate(members)]

        def run_group(n=total, store=False):
            s = DeviceGroupTemperedSampler(grp, [nw] * K, 6, betas=betas, seeds=seeds, chunk=a.chunk, rng='device')
            t = timed(grp.group, 'tempered_collect', lambda: s.run_mcmc(starts, n, store=store), a.skip) if n == total else s.run_mcmc(starts, n)
            return t, s

        def run_solo(n=total, only=None):
            t, last = 0.0, None
            for k, e in enumerate(members if only is None else members[:only]):
                last = DeviceTemperedSampler(nw, 6, e, betas=betas, seed=seeds[k], chunk=a.chunk, rng='device')
                if n == total:
                    t += timed(e.ctx, 'tempered_collect', lambda: last.run_mcmc(starts[k], n, store=False), a.skip)
                else:
                    last.run_mcmc(starts[k], n)
            return t, last

        # the warm-up round: the values first, then one untimed run of each driver
        _, g = run_group(2 * a.chunk + 3)
        _, one = run_solo(2 * a.chunk + 3, only=1)
        same = bool(np.array_equal(g.target(0).get_chain(t=None), one.get_chain(t=None)) and
                    np.array_equal(g.target(0).get_log_like(t=None), one.get_log_like(t=None)) and
                    np.array_equal(g.target(0).swap_fraction, one.swap_fraction))
        _, g = run_group()
        run_solo()
        rounds = {'group': [], 'solo': []}
        for r in range(a.rounds):
            for d in (('group', 'solo') if r % 2 == 0 else ('solo', 'group')):
                rounds[d].append((run_group if d == 'group' else run_solo)()[0])
        med = {d: float(np.median(v)) for d, v in rounds.items()}
        rec = {'what': 'group_tempered_us_per_iter', 'shape': name, 'targets': K, 'ntemps': T, 'walkers_per_rung': nw,
               'proposals_per_launch': K * T * nw // 2, 'iters': a.iters, 'skip': a.skip, 'chunk': a.chunk, 'beta_min': a.beta_min,
               'group_us_per_iter': med['group'], 'solo_sum_us_per_iter': med['solo'], 'ratio': med['group'] / med['solo'],
               'group_rounds': rounds['group'], 'solo_rounds': rounds['solo'],
               'group_spread': max(rounds['group']) - min(rounds['group']), 'solo_spread': max(rounds['solo']) - min(rounds['solo']),
               'target0_equals_its_solo_run': same,
               'swap_fraction_target0': [float(x) for x in g.target(0).swap_fraction],
               'acceptance_target0': [float(x) for x in g.target(0).acceptance_fraction.mean(axis=1)],
               'evaluations_per_second': 2.0 * K * T * nw / (med['group'] * 1e-6)}
        if name in GATED:
            rec['bar'] = BAR
            rec['meets_bar'] = bool(rec['ratio'] <= BAR)
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        grp.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')
    if not all(r.get('meets_bar', True) and r['target0_equals_its_solo_run'] for r in lines):
        sys.exit(1)


if __name__ == '__main__':
    main()
