"""Plain-Python restatements the moves tests compare with (mcmc_spec_amd.moves): one iteration of a
move over an ensemble, entry by entry and coordinate by coordinate, and the counter generator's packing in Python integers.
Nothing here is shared with the code under test."""
import math

import numpy as np

M64 = 0xffffffffffffffff
STRETCH, DE = 0, 1


def iterate(coords, logp, log_prob_fn, sidx, cidx, kind, p1, p2, g, fac, logu):
    """One iteration in the general layout (arrays of ONE iteration: sidx .. logu (2, ns), kind a number), in place on
    coords (nw, ndim) and logp (nw): returns the walkers that moved."""
    nw, ndim = coords.shape
    moved = np.zeros(nw, dtype=bool)
    for h in (0, 1):
        S, C = [int(i) for i in sidx[h]], [int(i) for i in cidx[h]]
        q = np.empty((len(S), ndim))
        for j, s in enumerate(S):
            c1, c2 = C[int(p1[h][j])], C[int(p2[h][j])]
            for d in range(ndim):
                sv = float(coords[s, d])
                if int(kind) == STRETCH:
                    cv = float(coords[c1, d])
                    diff = cv - sv
                    prod = diff * float(g[h][j])
                    q[j, d] = cv - prod
                else:
                    assert c1 != c2
                    diff = float(coords[c1, d]) - float(coords[c2, d])
                    prod = float(g[h][j]) * diff
                    q[j, d] = sv + prod
        new = np.asarray(log_prob_fn(q), dtype=float)
        for j, s in enumerate(S):
            lnpdiff = (float(fac[h][j]) + float(new[j])) - float(logp[s])   # (nan compares False)
            if float(logu[h][j]) < lnpdiff:
                coords[s] = q[j]
                logp[s] = new[j]
                moved[s] = True
    return moved


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


def uniform_int(seed, it, stream, index):
    return float(mix64_int(seed, it, stream, index) >> 11) * (1.0 / 9007199254740992.0)


def de_pair_int(u, nc):
    """The ordered pair of distinct indices below nc that a uniform u selects (section 1 of the moves' specification)."""
    npairs = nc * (nc - 1)
    p = min(int(math.floor(u * npairs)), npairs - 1)
    j1, r = p // (nc - 1), p % (nc - 1)
    return j1, r + (1 if r >= j1 else 0)
