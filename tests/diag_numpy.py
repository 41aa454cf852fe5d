"""NumPy restatement of msx_series_moments (include/msx.h; csrc/diag_kernels.h) with its exact
summation order -- ``twin`` -- and the definition written out as loops over ``math.fsum`` -- ``loops``.  Nothing here is
shared with the code under test.

The order (fixed by n' and the members' walker counts alone).  Per (walker, column, range) 256 "threads": thread i adds the
range's elements i, i + 256, ... one after the other starting from +0.0, then the 256 partial sums fold as a tree (128 + 128,
64 + 64, ...).  The ranges are half 0 = rows [0, h), half 1 = rows [n' - h, n') and all n' rows, h = n' // 2.  A member's
half-chains combine in the order j = 2 w + half, its walkers' totals and cross products in walker order.
"""
import math

import numpy as np

THREADS = 256   # kDiagThreads


def _fold(x):
    """x (W, cnt) -> (W,): the 256 strided sequences, then the tree."""
    W, cnt = x.shape
    acc = np.zeros((W, THREADS))
    for r0 in range(0, cnt, THREADS):
        seg = x[:, r0:r0 + THREADS]
        acc[:, :seg.shape[1]] = acc[:, :seg.shape[1]] + seg
    h = THREADS // 2
    while h > 0:
        acc[:, :h] = acc[:, :h] + acc[:, h:2 * h]
        h //= 2
    return acc[:, 0].copy()


def _seq(values):
    s = np.float64(0.0)
    for v in values:
        s = s + np.float64(v)
    return s


def twin(x, counts, cov=True):
    """x (n', nw, ncols): the selection.  {'within', 'var_plus', 'between', 'mean' (k, ncols), 'cov' (k, ncols, ncols) or
    None}: the device's arithmetic, operation for operation."""
    x = np.asarray(x, dtype=np.float64)
    n, _, nc = x.shape
    h = n // 2
    k = len(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    out = {name: np.empty((k, nc)) for name in ('within', 'var_plus', 'between', 'mean')}
    out['cov'] = np.empty((k, nc, nc)) if cov else None
    dh, dh1 = np.float64(h), np.float64(h - 1)
    with np.errstate(invalid='ignore', over='ignore', divide='ignore'):
        for m in range(k):
            W = int(counts[m])
            J, J1, N = np.float64(2 * W), np.float64(2 * W - 1), n * W
            xm = [np.ascontiguousarray(x[:, off[m]:off[m + 1], q].T) for q in range(nc)]   # (W, n') per column
            for q in range(nc):
                halves = (xm[q][:, :h], xm[q][:, n - h:])
                S = [_fold(p) for p in halves]                                    # [half](W,)
                mj = [s / dh for s in S]
                SS = [_fold((p - mj[i][:, None]) * (p - mj[i][:, None])) for i, p in enumerate(halves)]
                order = [(w, i) for w in range(W) for i in (0, 1)]                # j = 2 w + half
                mbar = _seq(mj[i][w] for w, i in order) / J
                within = _seq(SS[i][w] / dh1 for w, i in order) / J
                between = _seq((mj[i][w] - mbar) * (mj[i][w] - mbar) for w, i in order) / J1
                out['within'][m, q], out['between'][m, q] = within, between
                out['var_plus'][m, q] = (dh1 / dh) * within + between
                out['mean'][m, q] = _seq(_fold(xm[q])) / np.float64(N)
            if cov:
                for d in range(nc):
                    for e in range(d, nc):
                        a = xm[d] - out['mean'][m, d]
                        b = xm[e] - out['mean'][m, e]
                        v = _seq(_fold(a * b)) / np.float64(N - 1)
                        out['cov'][m, d, e] = out['cov'][m, e, d] = v
    return out


def loops(x, counts):
    """The definition as written-out loops with exactly rounded sums (``math.fsum``); finite data.  twin's dict plus 'rhat'."""
    x = np.asarray(x, dtype=np.float64)
    n, _, nc = x.shape
    h = n // 2
    k = len(counts)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    out = {name: np.empty((k, nc)) for name in ('within', 'var_plus', 'between', 'mean', 'rhat')}
    out['cov'] = np.empty((k, nc, nc))
    for m in range(k):
        W = int(counts[m])
        J = 2 * W
        for q in range(nc):
            ms, s2 = [], []
            for w in range(off[m], off[m + 1]):
                for rows in (range(0, h), range(n - h, n)):
                    v = [float(x[t, w, q]) for t in rows]
                    mj = math.fsum(v) / h
                    ms.append(mj)
                    s2.append(math.fsum((a - mj) ** 2 for a in v) / (h - 1))
            mbar = math.fsum(ms) / J
            within = math.fsum(s2) / J
            between = math.fsum((a - mbar) ** 2 for a in ms) / (J - 1)
            var_plus = (h - 1) / h * within + between
            out['within'][m, q], out['between'][m, q], out['var_plus'][m, q] = within, between, var_plus
            out['rhat'][m, q] = math.sqrt(var_plus / within) if within > 0.0 else math.nan
            out['mean'][m, q] = math.fsum(float(a) for a in x[:, off[m]:off[m + 1], q].ravel()) / (n * W)
        for d in range(nc):
            for e in range(nc):
                a = x[:, off[m]:off[m + 1], d].ravel() - out['mean'][m, d]
                b = x[:, off[m]:off[m + 1], e].ravel() - out['mean'][m, e]
                out['cov'][m, d, e] = math.fsum(float(p) * float(r) for p, r in zip(a, b)) / (n * W - 1)
    return out


def close(a, b, tol):
    """|a - b| <= tol |b| elementwise, equal infinities, NaN in the same places."""
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    same = (a == b) | (np.isnan(a) & np.isnan(b))
    with np.errstate(invalid='ignore'):
        near = np.abs(a - b) <= tol * np.abs(b)
    return bool(np.all(same | (np.isfinite(a) & np.isfinite(b) & near)))
