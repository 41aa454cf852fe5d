#!/usr/bin/env python3
"""Target groups against one launch per target, on the eight KOI targets of
tests/golden/golden_koi.npz, as JSON lines (and into the file named by --out):
  * launch_us: K = 1, 2, 4, 8 targets x 16, 25, 64, 512 walkers per target -- ONE group launch against the K targets'
    own launches queued back to back on one stream.  HIP events around `reps` repetitions, `rounds` alternating rounds,
    medians (and the rounds themselves);
  * sampler_ms: one host-driven GroupSampler iteration (8 targets x 50 walkers: the reference's example) against 8
    separate host EnsembleSamplers stepped one after another, wall time per iteration, median of the rounds.
Values are checked first: the group's bits equal the single launches'."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def koi_engines():
    from mcmc_spec_amd import bands
    from mcmc_spec_amd.engine import Engine
    import common
    from test_koi_config5 import koi_cases, koi_problem
    g, _ = koi_cases()
    c = common.golden_case('A')
    bl = bands.make_bands(c.tables, *c.vega)
    engines = []
    for tag in [str(t) for t in g['targets']]:
        data, err, fr, r, ctm, ptm, tmi, tma = koi_problem(g, tag)
        eng = Engine(0)
        eng.stage_specs(c.specs)
        eng.stage_problem(data, err, fr, r, ctm, ptm, tmi, tma, c.matrix, nspec=2, bands=bl,
                          av_table=common.av_table_exact(), tmin=c.tmin, tmax=c.tmax, prior=c.prior, rad_prior=True)
        engines.append(eng)
    return c, engines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=None)
    ap.add_argument('--reps', type=int, default=100)
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--sampler-iters', type=int, default=20)
    a = ap.parse_args()
    import torch  # (first: one HIP runtime per process, see mcmc_spec_amd/_lib.py)
    from mcmc_spec_amd import _lib, synth
    from mcmc_spec_amd.group import GroupSampler, TargetGroup
    from mcmc_spec_amd.sampler import EnsembleSampler
    c, engines = koi_engines()
    lines = []

    def out(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    s = torch.cuda.current_stream()
    mode = _lib.MODE_LOGPOST
    for K in (1, 2, 4, 8):
        grp = TargetGroup(engines[:K])
        for nw in (16, 25, 64, 512):
            ths = [synth.draw_walkers(nw, seed=100 * k + nw, tmin=c.tmin, tmax=c.tmax) for k in range(K)]
            flat = np.concatenate(ths)
            n = len(flat)
            d_th = torch.tensor(flat, device='cuda')
            lp = torch.empty(n, dtype=torch.float64, device='cuda')
            st = torch.empty(n, dtype=torch.int32, device='cuda')
            lp1 = torch.empty(n, dtype=torch.float64, device='cuda')
            st1 = torch.empty(n, dtype=torch.int32, device='cuda')
            counts = [nw] * K

            def group():
                grp.group.logprob_batch_dev(d_th.data_ptr(), counts, 6, lp.data_ptr(), st.data_ptr(), s.cuda_stream, mode)

            def singles():
                for k in range(K):
                    o = k * nw
                    engines[k].ctx.logprob_batch_dev(d_th.data_ptr() + 8 * 6 * o, nw, 6, lp1.data_ptr() + 8 * o,
                                                     st1.data_ptr() + 4 * o, s.cuda_stream, mode)
            group()
            singles()
            torch.cuda.synchronize()
            same = bool(torch.equal(lp.nan_to_num(nan=123.0), lp1.nan_to_num(nan=123.0)) and torch.equal(st, st1))
            if not same:
                raise SystemExit('group launch differs from the single launches (K={}, walkers={})'.format(K, nw))

            def timed(fn):
                for _ in range(10):
                    fn()
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(s)
                for _ in range(a.reps):
                    fn()
                e1.record(s)
                e1.synchronize()
                return e0.elapsed_time(e1) * 1e3 / a.reps
            g_us, s_us = [], []
            for _ in range(a.rounds):
                g_us.append(timed(group))
                s_us.append(timed(singles))
            gm, sm = float(np.median(g_us)), float(np.median(s_us))
            info = grp.launch_info(counts)
            out(dict(what='launch_us', targets=K, walkers_per_target=nw, group=gm, sequential=sm, ratio=gm / sm,
                     group_rounds=g_us, sequential_rounds=s_us, kernel=info['kernel']))
        grp.close()

    # host-driven lock-step sampler against separate host samplers, 8 targets x 50 walkers
    K, nw = 8, 50
    grp = TargetGroup(engines)
    p0s = [synth.draw_walkers(nw, seed=900 + k, tmin=c.tmin, tmax=c.tmax) for k in range(K)]
    g_ms, s_ms = [], []
    for r in range(a.rounds):
        gs = GroupSampler([nw] * K, 6, grp.logposterior, seeds=list(range(K)))
        st = gs.run_mcmc(p0s, 2)
        t0 = time.perf_counter()
        gs.run_mcmc(st, a.sampler_iters)
        g_ms.append((time.perf_counter() - t0) * 1e3 / a.sampler_iters)
        es = [EnsembleSampler(nw, 6, engines[k].logposterior, vectorize=True, seed=k) for k in range(K)]
        sts = [e.run_mcmc(p0s[k], 2) for k, e in enumerate(es)]
        gens = [e.sample(sts[k], iterations=a.sampler_iters) for k, e in enumerate(es)]
        t0 = time.perf_counter()
        for _ in range(a.sampler_iters):
            for gen in gens:
                next(gen)
        s_ms.append((time.perf_counter() - t0) * 1e3 / a.sampler_iters)
    out(dict(what='sampler_ms_per_iteration', targets=K, walkers_per_target=nw, group_sampler=float(np.median(g_ms)),
             separate_samplers=float(np.median(s_ms)), group_rounds=g_ms, separate_rounds=s_ms))
    if a.out:
        with open(a.out, 'w') as fh:
            fh.write(''.join(json.dumps(r) + '\n' for r in lines))


if __name__ == '__main__':
    main()
