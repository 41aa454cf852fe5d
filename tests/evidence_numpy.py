"""NumPy restatement of msx_series_evidence (include/msx.h; csrc/evidence_kernels.h) with its exact
summation order -- ``twin`` -- and an independent reference built on ``math.fsum`` -- ``reference``.  Nothing here is shared
with the code under test.

The order (fixed by n', W_m and B alone).  The selection x = rows[0:n][discard::thin] of one column is cut into B blocks,
block b = rows floor(b n' / B) .. floor((b + 1) n' / B) - 1.  Per (walker, block) 256 "threads": thread i adds the block's
elements i, i + 256, ... one after the other starting from +0.0, then the 256 partial sums fold as a tree (128 + 128, 64 +
64, ...).  The walkers' sums of a member are added in walker order, the blocks' in block order.  The maximum ignores NaN.
"""
import math

import numpy as np

THREADS = 256      # kEvdThreads: the stride through a block and the width of the tree (the kernel's tile)
MAX_BLOCKS = 64    # kEvdMaxBlocks


def bounds(n, B):
    return [b * n // B for b in range(B + 1)]


def _max(a, b):
    return np.where(b > a, b, a)   # (a NaN in b is ignored; a is never NaN)


def _fold(x, op, init):
    """x (W, cnt) -> (W,): the 256 strided sequences, then the tree."""
    W, cnt = x.shape
    acc = np.full((W, THREADS), init, dtype=np.float64)
    for r0 in range(0, cnt, THREADS):
        seg = x[:, r0:r0 + THREADS]
        acc[:, :seg.shape[1]] = op(acc[:, :seg.shape[1]], seg)
    h = THREADS // 2
    while h > 0:
        acc[:, :h] = op(acc[:, :h], acc[:, h:2 * h])
        h //= 2
    return acc[:, 0].copy()


def _seq(values):
    s = 0.0
    for v in values:
        s = s + float(v)
    return s


def _lme(d, M, S, N):
    if S == 0.0:
        return -math.inf
    with np.errstate(invalid='ignore', divide='ignore'):
        return float(np.float64(d) * np.float64(M) + np.log(np.float64(S) / np.float64(N)))


def twin(x, counts, db, B):
    """x (n', nw): the selected rows of the column; counts: the members' walker counts; db (k,) or None.  (mean, lme),
    each (k, B + 1); lme None without db."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    lo = bounds(n, B)
    k = len(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    mean = np.empty((k, B + 1))
    lme = None if db is None else np.empty((k, B + 1))
    with np.errstate(invalid='ignore', over='ignore'):
        for m in range(k):
            W = int(counts[m])
            xm = np.ascontiguousarray(x[:, off[m]:off[m + 1]].T)   # (W, n')
            bsum, bmax, bexp = [], [], []
            for b in range(B):
                blk = xm[:, lo[b]:lo[b + 1]]
                s = _seq(_fold(blk, np.add, 0.0))
                M = -math.inf
                for v in _fold(blk, _max, -np.inf):
                    M = float(v) if v > M else M
                bsum.append(s)
                bmax.append(M)
                mean[m, 1 + b] = np.float64(s) / np.float64((lo[b + 1] - lo[b]) * W)
            mean[m, 0] = np.float64(_seq(bsum)) / np.float64(n * W)
            if db is None:
                continue
            d = np.float64(db[m])
            for b in range(B):
                blk = xm[:, lo[b]:lo[b + 1]]
                diff = blk - np.float64(bmax[b])
                arg = d * diff
                e = np.where(blk == -np.inf, 0.0, np.exp(arg))
                S = _seq(_fold(e, np.add, 0.0))
                bexp.append(S)
                lme[m, 1 + b] = _lme(d, bmax[b], S, (lo[b + 1] - lo[b]) * W)
            M = -math.inf
            for v in bmax:
                M = v if v > M else M
            S = 0.0
            for b in range(B):
                diff = np.float64(bmax[b]) - np.float64(M)
                term = np.float64(bexp[b]) * np.exp(d * diff)
                S = S + (0.0 if bexp[b] == 0.0 else float(term))
            lme[m, 0] = _lme(d, M, S, n * W)
    return mean, lme


def _ref_mean(v):
    v = [float(a) for a in v]
    if any(math.isnan(a) for a in v):
        return math.nan
    if any(a == -math.inf for a in v):
        return -math.inf
    return math.fsum(v) / len(v)


def _ref_lme(v, d):
    v = [float(a) for a in v]
    if any(math.isnan(a) for a in v):
        return math.nan
    fin = [a for a in v if a != -math.inf]
    if not fin:
        return -math.inf
    M = max(fin)
    return d * M + math.log(math.fsum(math.exp(d * (a - M)) for a in fin) / len(v))


def reference(x, counts, db, B):
    """The same quantities from ``math.fsum`` (exactly rounded sums) and a logsumexp built on it; no +inf in x."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    lo = bounds(n, B)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    mean = np.empty((len(counts), B + 1))
    lme = None if db is None else np.empty((len(counts), B + 1))
    for m in range(len(counts)):
        xm = x[:, off[m]:off[m + 1]]
        parts = [xm] + [xm[lo[b]:lo[b + 1]] for b in range(B)]
        for j, p in enumerate(parts):
            mean[m, j] = _ref_mean(p.ravel())
            if db is not None:
                lme[m, j] = _ref_lme(p.ravel(), float(db[m]))
    return mean, lme


def close(a, b, tol):
    """|a - b| <= tol max(1, |b|) elementwise, equal infinities and NaN in the same places."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid='ignore'):
        near = np.abs(a - b) <= tol * np.maximum(1.0, np.abs(b))
    return bool(np.all(same | (np.isfinite(a) & np.isfinite(b) & near)))
