#!/usr/bin/env python3
"""What rank-normalised R-hat and bulk / tail ESS cost on a resident series, as JSON lines (and into
--out, default profiles/ess_bench.jsonl), in one process on one GPU.  Two shapes -- one chain of 50 walkers x 15,000 rows x 6
columns, and 8 members x 256 walkers x 15,000 rows x 6 -- and two sides that ALTERNATE inside every block after a warm-up:
  * device: ``Series.rank_stats(want=('rhat', 'bulk', 'tail'))`` -- what a stopping rule asks for -- and, on its own, the sort
    alone (``split_transform`` to twice the ranks); a host clock around the synchronous calls;
  * host: the download (``Series.read``) and then ``diagnostics.rank_rhat`` + ``diagnostics.ess`` ('bulk', 'tail') on the
    array.  At the large shape the definition is timed on member 0's column 0 alone and multiplied by the 48 segments
    (``host_extrapolated``).
A block is --reps alternations; the figures are the medians over the 3 blocks of each block's median.  The sort's traffic is
counted from the passes the data needs (a digit that is the same all over every segment of a round is dropped): per pass and
value 8 bytes read for the counts, 12 read and 12 written by the scatter."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ROWS, NDIM = 15000, 6
SHAPES = (('one chain', [50]), ('8 x 256', [256] * 8))
BLOCKS = 3
WANT = ('rhat', 'bulk', 'tail')


def clock(fn):
    t0 = time.perf_counter()
    res = fn()
    return 1e3 * (time.perf_counter() - t0), res


def passes_needed(rows, counts):
    """The byte positions of the keys that differ somewhere in some (member, column) of the split pool (all rows: n' even)."""
    need = np.zeros(8, dtype=bool)
    off = np.concatenate([[0], np.cumsum(counts)])
    for m in range(len(counts)):
        for c in range(rows.shape[2]):
            b = np.ascontiguousarray(rows[:, off[m]:off[m + 1], c]).view(np.uint8).reshape(-1, 8)
            need |= b.min(axis=0) != b.max(axis=0)
    return int(need.sum())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'ess_bench.jsonl'))
    ap.add_argument('--reps', type=int, default=3, help='alternations per block')
    ap.add_argument('--rows', type=int, default=ROWS)
    a = ap.parse_args()
    import torch  # noqa: F401  (first: one HIP runtime per process, see mcmc_spec_amd/_lib.py)
    from mcmc_spec_amd import _lib, diagnostics
    from mcmc_spec_amd.engine import Engine
    ctx = Engine(0).ctx
    lines = []
    for name, counts in SHAPES:
        nw, large = sum(counts), len(counts) > 1
        rng = np.random.default_rng(len(counts))
        ser = _lib.Series(ctx, nw, NDIM, counts, cap_hint=a.rows)
        centre, scale = np.array([5800.0, 3400.0, 0.3, 0.05, 0.02, 1e-4]), np.array([40.0, 60.0, 0.02, 0.01, 0.004, 2e-5])
        state = rng.normal(size=(nw, NDIM))
        for b in range(0, a.rows, 1000):   # AR(1) at rho = 0.95 per walker and column: correlated rows, a stationary spread
            m = min(1000, a.rows - b)
            e = rng.normal(size=(m, nw, NDIM)) * np.sqrt(1.0 - 0.95 ** 2)
            x = np.empty_like(e)
            for i in range(m):
                state = 0.95 * state + e[i]
                x[i] = state
            ser.append(centre + scale * x)
        sel = (slice(None), slice(0, counts[0]), slice(0, 1)) if large else (slice(None),) * 3
        segments = len(counts) * NDIM

        def host():
            t_read, rows = clock(lambda: ser.read(0, a.rows))
            part = rows[sel]
            t_calc, res = clock(lambda: (diagnostics.rank_rhat(part, [part.shape[1]]), diagnostics.ess(part, 'bulk', [part.shape[1]]),
                                         diagnostics.ess(part, 'tail', [part.shape[1]])))
            return t_read, t_calc * (segments if large else 1), res, rows

        device = lambda: ser.rank_stats(a.rows, want=WANT)
        dst = ser.split_sibling(NDIM)
        sort = lambda: ser.split_transform(a.rows, 0, 1, range(NDIM), _lib.SPLIT_RANK2, dst)
        device(), sort()
        _, _, _, rows = host()
        npass = passes_needed(rows, counts)
        del rows
        blocks = {k: [] for k in ('device', 'sort', 'download', 'host')}
        dev = res = None
        for _ in range(BLOCKS):
            ms = {k: [] for k in blocks}
            for _ in range(1 if large else a.reps):
                t, dev = clock(device)
                ms['device'].append(t)
                t, _ = clock(sort)
                ms['sort'].append(t)
                t_read, t_calc, res, _ = host()
                ms['download'].append(t_read)
                ms['host'].append(t_calc)
            for k in blocks:
                blocks[k].append(float(np.median(ms[k])))
        dst.close()
        rr, bulk, tail = res
        rel = lambda x, y: bool(np.all(np.abs(x - y) <= 1e-9 * np.abs(y)))
        pick = (lambda v: v[:1, :1]) if large else (lambda v: v)
        agree = all(rel(pick(dev[k]), rr[k]) for k in ('bulk', 'folded', 'rhat')) and rel(pick(dev['ess_bulk']), bulk) and rel(pick(dev['ess_tail']), tail)
        med = {k: float(np.median(v)) for k, v in blocks.items()}
        values = a.rows * nw * NDIM
        rec = {'what': 'rank_rhat_bulk_tail_ess', 'shape': name, 'members': len(counts), 'walkers': nw, 'rows': a.rows, 'ndim': NDIM,
               'values': values, 'reps': 1 if large else a.reps, 'blocks': BLOCKS, 'device_ms': med['device'], 'sort_ms': med['sort'],
               'sorts_per_device_call': 2, 'sort_share': 2 * med['sort'] / med['device'], 'sort_passes': npass,
               'sort_gb_per_s': 32.0 * values * npass / (med['sort'] * 1e-3) / 1e9, 'download_ms': med['download'], 'host_ms': med['host'],
               'host_extrapolated': large, 'host_with_download_ms': med['download'] + med['host'],
               'speedup_with_download': (med['download'] + med['host']) / med['device'], 'agree': agree,
               'min_ess_bulk': float(np.min(dev['ess_bulk'])), 'max_rank_rhat': float(np.max(dev['rhat'])), 'block_medians_ms': blocks}
        print(json.dumps(rec), flush=True)
        lines.append(rec)
        ser.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as f:
            for rec in lines:
                f.write(json.dumps(rec) + '\n')


if __name__ == '__main__':
    main()
