"""Plain-Python restatements the tempering tests compare with (mcmc_spec_amd.tempered): one iteration
of a ladder -- rung by rung, walker by walker, coordinate by coordinate, Python floats -- and its swap sweep; the packing of
the swap draws' counter (stream 14) in Python integers.  Nothing here is shared with the code under test."""
import math

import numpy as np

M64 = 0xffffffffffffffff
STRETCH, DE = 0, 1
SWAP_STREAM, SWAP_STRIDE = 14, 4096


def density(beta, lpr, ll):
    """P_t = lpr + beta * ll in two roundings (Python floats are float64; no contraction)."""
    prod = float(beta) * float(ll)
    return float(lpr) + prod


def iterate(betas, coords, ll, lpr, loglike_fn, logprior_fn, members):
    """One iteration's two half-steps of every rung, in place on coords (T, nw, ndim), ll, lpr (T, nw).  members[t]: the
    general layout of ONE iteration of rung t (sidx .. logu (2, ns), kind a number).  Returns the walkers that moved."""
    T, nw, ndim = coords.shape
    moved = np.zeros((T, nw), dtype=bool)
    for h in (0, 1):
        for t in range(T):
            sidx, cidx, kind, p1, p2, g, fac, logu = members[t]
            S, C = [int(i) for i in sidx[h]], [int(i) for i in cidx[h]]
            q = np.empty((len(S), ndim))
            for j, s in enumerate(S):
                c1, c2 = C[int(p1[h][j])], C[int(p2[h][j])]
                for d in range(ndim):
                    sv = float(coords[t, s, d])
                    if int(kind) == STRETCH:
                        cv = float(coords[t, c1, d])
                        diff = cv - sv
                        prod = diff * float(g[h][j])
                        q[j, d] = cv - prod
                    else:
                        assert c1 != c2
                        diff = float(coords[t, c1, d]) - float(coords[t, c2, d])
                        prod = float(g[h][j]) * diff
                        q[j, d] = sv + prod
            new_lpr = np.asarray(logprior_fn(q), dtype=float)
            new_ll = np.asarray(loglike_fn(q), dtype=float)
            for j, s in enumerate(S):
                p_q = density(betas[t], new_lpr[j], new_ll[j])
                p_s = density(betas[t], lpr[t, s], ll[t, s])
                lnpdiff = (float(fac[h][j]) + p_q) - p_s     # (nan compares False)
                if float(logu[h][j]) < lnpdiff:
                    coords[t, s] = q[j]
                    ll[t, s] = new_ll[j]
                    lpr[t, s] = new_lpr[j]
                    moved[t, s] = True
    return moved


def sweep(betas, coords, ll, lpr, swap_logu):
    """The swap sweep of one iteration, in place; swap_logu (T - 1, nw), row p for the pair (p + 1, p).  Returns the swaps
    accepted per pair, a list of T - 1 integers."""
    T, nw, ndim = coords.shape
    count = [0] * (T - 1)
    for w in range(nw):
        for t in range(T - 1, 0, -1):
            d = float(ll[t, w]) - float(ll[t - 1, w])
            db = float(betas[t - 1]) - float(betas[t])
            lnr = db * d
            if float(swap_logu[t - 1][w]) < lnr:
                for k in range(ndim):
                    coords[t, w, k], coords[t - 1, w, k] = float(coords[t - 1, w, k]), float(coords[t, w, k])
                ll[t, w], ll[t - 1, w] = float(ll[t - 1, w]), float(ll[t, w])
                lpr[t, w], lpr[t - 1, w] = float(lpr[t - 1, w]), float(lpr[t, w])
                count[t - 1] += 1
    return count


def mix64_int(seed, it, stream, index):
    """SplitMix64's output function over the counter (it << 28) + (stream << 24) + index, in Python integers."""
    assert 0 <= index < 1 << 24 and 0 <= stream < 1 << 4 and 0 <= it < 1 << 36
    ctr = (it << 28) + (stream << 24) + index
    x = ((seed & M64) * 0xD1342543DE82EF95 + (ctr + 1) * 0x9E3779B97F4A7C15) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def swap_index(t, w):
    """The index field of the swap draw of the pair (t, t - 1) at walker w."""
    assert 1 <= t <= 63 and 0 <= w < SWAP_STRIDE
    return (t - 1) * SWAP_STRIDE + w


def swap_uniform_int(seed0, it, t, w):
    return float(mix64_int(seed0, it, SWAP_STREAM, swap_index(t, w)) >> 11) * (1.0 / 9007199254740992.0)


def swap_logu_int(seed0, first_iter, m, T, nw):
    """ln u (m, T - 1, nw) of the device's swap draws, entry by entry."""
    out = np.empty((m, T - 1, nw))
    for i in range(m):
        for t in range(1, T):
            for w in range(nw):
                u = swap_uniform_int(seed0, first_iter + i, t, w)
                out[i, t - 1, w] = math.log(u) if u > 0.0 else -math.inf
    return out


def run(betas, p0, loglike_fn, logprior_fn, nsteps, seed, a=2.0):
    """A whole tempered run with the stretch move from generators of its own (not the samplers' streams): what each rung
    samples, for the statistical tests' run lengths.  Returns (chain (nsteps, T, nw, ndim), swaps per pair)."""
    rng = np.random.default_rng(seed)
    betas = np.asarray(betas, dtype=float)
    T = len(betas)
    nw, ndim = p0.shape
    ns = nw // 2
    coords = np.repeat(p0[None], T, axis=0).copy()
    flat = coords.reshape(-1, ndim)
    ll = np.asarray(loglike_fn(flat), dtype=float).reshape(T, nw).copy()
    lpr = np.asarray(logprior_fn(flat), dtype=float).reshape(T, nw).copy()
    chain = np.empty((nsteps, T, nw, ndim))
    nswap = np.zeros(T - 1, dtype=np.int64)
    for i in range(nsteps):
        for t in range(T):
            perm = rng.permutation(nw)
            for h in (0, 1):
                S, C = (perm[:ns], perm[ns:]) if h == 0 else (perm[ns:], perm[:ns])
                z = ((a - 1.0) * rng.random(ns) + 1.0) ** 2 / a
                c = coords[t, C[rng.integers(0, ns, ns)]]
                q = c - (c - coords[t, S]) * z[:, None]
                lq, pq = np.asarray(loglike_fn(q), dtype=float), np.asarray(logprior_fn(q), dtype=float)
                with np.errstate(invalid='ignore'):
                    d = ((ndim - 1.0) * np.log(z) + (pq + betas[t] * lq)) - (lpr[t, S] + betas[t] * ll[t, S])
                acc = np.log(rng.random(ns)) < d
                coords[t, S[acc]], ll[t, S[acc]], lpr[t, S[acc]] = q[acc], lq[acc], pq[acc]
        for t in range(T - 1, 0, -1):
            with np.errstate(invalid='ignore'):
                sw = np.log(rng.random(nw)) < (betas[t - 1] - betas[t]) * (ll[t] - ll[t - 1])
            nswap[t - 1] += sw.sum()
            for arr in (coords, ll, lpr):
                tmp = arr[t, sw].copy()
                arr[t, sw] = arr[t - 1, sw]
                arr[t - 1, sw] = tmp
        chain[i] = coords
    return chain, nswap
