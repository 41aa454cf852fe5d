"""Plain-Python restatements the adaptive-ladder tests compare with (mcmc_spec_amd.tempered.ladder_step; DESIGN.md section
19): the ladder's exponential and one ladder step, rung by rung in Python floats, and the adaptive loop -- the fixed ladder's
iteration and sweep of tests/tempered_numpy.py, then the step.  Nothing here is shared with the code under test."""
import math

import numpy as np

import tempered_numpy as tn


def exp_plain(x):
    """exp for |x| <= 1: the degree-12 Taylor polynomial in x / 8, Horner from the top with c[k] = 1 / k!, squared thrice."""
    y = float(x) * 0.125
    p = 1.0 / math.factorial(12)
    for k in range(11, -1, -1):
        p = p * y
        p = p + 1.0 / math.factorial(k)
    for _ in range(3):
        p = p * p
    return p


def ladder_step_plain(betas, counts, nw, k, lag, time):
    """(betas', skipped): one ladder step, every operation one rounding of Python floats in the definition's order."""
    b = [float(v) for v in betas]
    T = len(b)
    if T <= 2:
        return b, 0
    r = [float(int(c)) / float(nw) for c in counts]
    decay = float(lag) / (float(k) + float(lag))
    kappa = decay / float(time)
    Ti = [1.0 / v for v in b]
    g = [0.0] * T
    for p in range(1, T):
        g[p] = Ti[p] - Ti[p - 1]
    for p in range(1, T - 1):
        dS = kappa * (r[p - 1] - r[p])
        assert abs(dS) <= 1.0
        g[p] = g[p] * exp_plain(dS)
    c = [0.0] * T
    c[1] = g[1]
    for p in range(2, T):
        c[p] = c[p - 1] + g[p]
    span = Ti[T - 1] - Ti[0]
    out = list(b)
    for p in range(1, T - 1):
        den = Ti[0] + span * (c[p] / c[T - 1]) if c[T - 1] != 0.0 else math.nan
        out[p] = 1.0 / den if den != 0.0 else math.inf
    ok = all(math.isfinite(v) for v in out) and all(out[t] < out[t - 1] for t in range(1, T))
    return (out, 0) if ok else (b, 1)


def adaptive_run(betas, coords, ll, lpr, loglike_fn, logprior_fn, draw, m, k, lag, time):
    """m adaptive iterations in place on coords (T, nw, ndim), ll, lpr (T, nw).  ``draw()`` gives one iteration's
    ``(members, swap_logu)`` as ``TemperedSampler._draw_steps(1)`` does.  Returns the rows (chain, ll, lpr, the ladder each
    iteration ran WITH), the final ladder, the swaps per pair, the walkers' accept counts, the new k and the skipped steps."""
    T, nw, _ = coords.shape
    betas = [float(v) for v in betas]
    rows = ([], [], [], [])
    nswap, nacc, skipped = np.zeros(T - 1, dtype=np.int64), np.zeros((T, nw)), 0
    for _ in range(m):
        members, swap_logu = draw()
        one = [tuple(a[0] for a in mem) for mem in members]
        nacc += tn.iterate(betas, coords, ll, lpr, loglike_fn, logprior_fn, one)
        counts = tn.sweep(betas, coords, ll, lpr, swap_logu[0])
        nswap += np.array(counts, dtype=np.int64)
        for dst, src in zip(rows, (coords, ll, lpr, np.array(betas))):
            dst.append(np.array(src, dtype=float))
        betas, skip = ladder_step_plain(betas, counts, nw, k, lag, time)
        k += 1
        skipped += skip
    return [np.array(a) for a in rows], np.array(betas), nswap, nacc, k, skipped
