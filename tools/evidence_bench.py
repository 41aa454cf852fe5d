#!/usr/bin/env python3
"""What the ladder's device series and the evidence reduction cost, as JSON lines (and into --out,
default profiles/evidence_bench.jsonl), in one process on one GPU:
  * evidence: msx_series_evidence (8 blocks, the stepping stone's db) on 8 members x 256 walkers x 15,000 rows of (ll, lpr)
    against NumPy on the downloaded array -- tempered.host_evidence -- with the download (Series.read) timed separately and
    included; tools/summary_bench.py's method: the device's median of --reps calls after a warm-up, the host's best of up to
    3; the two results compared (means to 1e-12 relative, lme to 1e-12 max(1, |value|));
  * attached_us_per_iter: a T = 8 x 256 tempered run on config 2's problem with both series attached (autocorr='device')
    against the same run unattached (autocorr='host'), both storing their chains, device-drawn, stretch move;
    tools/tempered_bench.py's method: the clock runs between the completions of two chunks of a run that keeps two chunks
    queued, the variants alternate in one process after a warm-up round, medians over --rounds rounds."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))

K, WPM, ROWS, BLOCKS = 8, 256, 15000, 8


def timed_ms(fn, reps):
    ms, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = fn()
        ms.append(1e3 * (time.perf_counter() - t0))
    return ms, res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'evidence_bench.jsonl'))
    ap.add_argument('--reps', type=int, default=7)
    ap.add_argument('--iters', type=int, default=1024, help='timed iterations per run')
    ap.add_argument('--skip', type=int, default=256, help='iterations of a run before the clock starts')
    ap.add_argument('--rounds', type=int, default=5)
    ap.add_argument('--chunk', type=int, default=64)
    ap.add_argument('--beta-min', type=float, default=0.02)
    a = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process, see mcmc_spec_amd/_lib.py)
    import bench
    from mcmc_spec_amd import _lib, synth, tempered
    from mcmc_spec_amd.engine import Engine
    from tempered_bench import timed
    lines = []

    def out(rec):
        print(json.dumps(rec), flush=True)
        lines.append(rec)

    eng = Engine(0)
    ctx = eng.ctx

    # ---- (a) the reduction ----
    nw = K * WPM
    betas = tempered.default_betas(K, a.beta_min)
    db = tempered._ss_db(betas, list(range(K)))
    rng = np.random.default_rng(8)
    ser = _lib.Series(ctx, nw, 2, [WPM] * K, cap_hint=ROWS)
    host_rows = np.empty((ROWS, nw, 2))
    for b in range(0, ROWS, 1000):   # ln L falling and widening down the ladder, as a run's does
        x = np.stack([-3.0 / np.repeat(betas, WPM) * rng.chisquare(6, (1000, nw)) / 6.0 - 2000.0, rng.normal(-20.0, 1.0, (1000, nw))], axis=2)
        ser.append(x)
        host_rows[b:b + 1000] = x
    dev_fn = lambda: ser.evidence(ROWS, 0, 1, 0, db, BLOCKS)
    mean_fn = lambda: ser.evidence(ROWS, 0, 1, 0, None, BLOCKS)
    dev_fn()
    dev_ms, dev = timed_ms(dev_fn, a.reps)
    mean_ms, _ = timed_ms(mean_fn, a.reps)
    read_ms, got = timed_ms(lambda: ser.read(0, ROWS), 3)
    assert np.array_equal(got, host_rows)
    host_ms, host = timed_ms(lambda: tempered.host_evidence(got[:, :, 0].reshape(ROWS, K, WPM), db, BLOCKS), 3)
    same = bool(np.all(np.abs(dev[0] - host[0]) <= 1e-12 * np.abs(host[0])) and
                np.all(np.abs(dev[1] - host[1]) <= 1e-12 * np.maximum(1.0, np.abs(host[1]))))
    values = ROWS * nw
    out({'what': 'evidence', 'members': K, 'walkers': nw, 'rows': ROWS, 'blocks': BLOCKS, 'values': values,
         'device_ms': float(np.median(dev_ms)), 'device_means_only_ms': float(np.median(mean_ms)), 'download_ms': float(np.min(read_ms)),
         'host_ms': float(np.min(host_ms)), 'host_with_download_ms': float(np.min(host_ms) + np.min(read_ms)),
         'speedup': float(np.min(host_ms) / np.median(dev_ms)), 'speedup_with_download': float((np.min(host_ms) + np.min(read_ms)) / np.median(dev_ms)),
         'agree': same, 'stream_bytes': 2 * values * 8, 'gb_per_s': float(2 * values * 8 / (np.median(dev_ms) * 1e-3) / 1e9),
         'download_bytes': int(got.nbytes), 'device_ms_all': dev_ms, 'host_ms_all': host_ms, 'download_ms_all': read_ms})
    ser.close()
    del host_rows, got

    # ---- (b) the attached run ----
    W = bench.build_workload(eng, 4096, False)
    total = a.skip + a.iters
    p = synth.draw_walkers(K * WPM, seed=5 + K * WPM, tmin=W['tmin'], tmax=W['tmax'])
    start = tempered.TemperedState(p.reshape(K, WPM, 6), eng.loglikelihood(p).reshape(K, WPM), eng.logprior(p).reshape(K, WPM))

    def run(mode):
        s = tempered.DeviceTemperedSampler(WPM, 6, eng, betas=betas, seed=17, chunk=a.chunk, rng='device', autocorr=mode, cap_hint=total)
        t = timed(ctx, 'tempered_collect', lambda: s.run_mcmc(start, total), a.skip)
        ev = s.log_evidence(blocks=BLOCKS) if mode == 'device' else None
        return t, ev

    names = ['host', 'device']
    for n in names:
        run(n)   # warm-up round
    rounds = {n: [] for n in names}
    ev = None
    for r in range(a.rounds):
        for n in names[r % 2:] + names[:r % 2]:
            t, e = run(n)
            rounds[n].append(t)
            ev = e or ev
    base = float(np.median(rounds['host']))
    for n in names:
        rec = {'what': 'attached_us_per_iter', 'autocorr': n, 'shape': 'config2', 'ntemps': K, 'walkers_per_rung': WPM, 'iters': a.iters,
               'skip': a.skip, 'chunk': a.chunk, 'us_per_iter': float(np.median(rounds[n])), 'rounds': rounds[n],
               'spread': max(rounds[n]) - min(rounds[n]), 'ratio_to_unattached': float(np.median(rounds[n])) / base}
        if n == 'device':
            rec.update({'log_z': ev.log_z, 'mc_error': ev.mc_error, 'ladder_error': ev.ladder_error})
        out(rec)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
