"""Moves of the ensemble samplers, and sets of them (emcee 3's ``moves=`` argument).

``StretchMove(a)`` is the affine-invariant stretch move of Goodman & Weare (2010), the samplers' default.  ``DEMove(sigma,
gamma0)`` is the differential-evolution move of ter Braak (2006) in the form emcee 3 ships: a walker ``s`` of the active
half proposes ``q = s + g (c1 - c2)`` with ``c1 != c2`` two walkers of the complementary half, ``g = g0 (1 + sigma n)``,
``n`` a standard normal deviate and ``g0 = gamma0`` or ``2.38 / sqrt(2 ndim)``; the proposal is symmetric, so the accept
rule carries no factor.  ``DEMove(gamma0=1.0)`` is the mode-jumping variant: the difference of a walker in each mode
carries ``s`` across.  (The snooker move needs three sub-ensembles and is not provided.)

A set of moves is what ``moves=`` takes: one move, a list of moves (equal weights) or a list of ``(move, weight)``.  Each
ITERATION chooses one move of the set, for both of its half-steps, with the set's normalised weights -- emcee's rule.

The general layout of an iteration's randomness (``EnsembleSampler._draw_steps`` with a set; ``draws=`` callbacks):
``sidx, cidx`` (m, 2, ns) int32, ``kind`` (m,) int32, ``p1, p2`` (m, 2, ns) int32 indices into the complementary half,
``g, fac, logu`` (m, 2, ns) float64.  Stretch entries carry ``p1 = p2 = partner``, ``g = z``, ``fac = (ndim - 1) ln z``;
DE entries ``fac = 0``.  ``counter_draws_moves`` restates the device generator for a set in NumPy.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

MOVE_STRETCH, MOVE_DE, MAX_MOVES = 0, 1, 4   # include/msx.h MSX_MOVE_STRETCH, MSX_MOVE_DE, MSX_MAX_MOVES


class MsxMoveSet(C.Structure):
    """Mirror of ``msx_move_set`` (include/msx.h) -- keep the field order identical."""
    _fields_ = [('n', C.c_int32), ('kind', C.c_int32 * MAX_MOVES), ('weight', C.c_double * MAX_MOVES),
                ('a', C.c_double * MAX_MOVES), ('gamma0', C.c_double * MAX_MOVES), ('sigma', C.c_double * MAX_MOVES)]


class StretchMove:
    """``q = c - (c - s) z``, ``z = ((a - 1) u + 1)^2 / a``, factor ``(ndim - 1) ln z``."""
    kind = MOVE_STRETCH

    def __init__(self, a=2.0):
        self.a = float(a)
        if not (np.isfinite(self.a) and self.a > 1.0):
            raise ValueError('StretchMove: the stretch scale a must be > 1')

    def __repr__(self):
        return 'StretchMove(a={})'.format(self.a)


class DEMove:
    """``q = s + g (c1 - c2)``, ``g = g0 (1 + sigma n)``; ``gamma0=None``: ``g0 = 2.38 / sqrt(2 ndim)``; factor 0."""
    kind = MOVE_DE

    def __init__(self, sigma=1.0e-5, gamma0=None):
        self.sigma = float(sigma)
        self.gamma0 = None if gamma0 is None else float(gamma0)
        if not np.isfinite(self.sigma) or self.sigma < 0.0:
            raise ValueError('DEMove: sigma must be finite and >= 0')
        if self.gamma0 is not None and not (np.isfinite(self.gamma0) and self.gamma0 > 0.0):
            raise ValueError('DEMove: gamma0 must be finite and > 0 (None: 2.38 / sqrt(2 ndim))')

    def __repr__(self):
        return 'DEMove(sigma={}, gamma0={})'.format(self.sigma, self.gamma0)


class MoveSet:
    """A parsed ``moves=`` argument: the moves, their normalised weights and the cumulative weights the choice compares
    against (``np.cumsum``: a sequential sum, as the device adds them)."""

    def __init__(self, moves, weights):
        self.moves = list(moves)
        w = np.asarray(weights, dtype=np.float64)
        self.weights = w / w.sum()
        self.cum = np.cumsum(self.weights)

    def __len__(self):
        return len(self.moves)

    @property
    def kinds(self):
        return [m.kind for m in self.moves]

    @property
    def pure_stretch(self):
        return all(m.kind == MOVE_STRETCH for m in self.moves)

    def gamma0(self, i, ndim):
        g = self.moves[i].gamma0
        return 2.38 / np.sqrt(2.0 * float(ndim)) if g is None else g

    def as_struct(self):
        """The set as ``msx_move_set`` (gamma0 <= 0 stands for 2.38 / sqrt(2 ndim))."""
        s = MsxMoveSet()
        s.n = len(self.moves)
        for i, m in enumerate(self.moves):
            s.kind[i] = m.kind
            s.weight[i] = float(self.weights[i])
            s.a[i] = m.a if m.kind == MOVE_STRETCH else 2.0
            s.gamma0[i] = (m.gamma0 or 0.0) if m.kind == MOVE_DE else 0.0
            s.sigma[i] = m.sigma if m.kind == MOVE_DE else 0.0
        return s


def parse_moves(moves):
    """``moves=`` in emcee's three forms -> MoveSet: one move, a list of moves (equal weights), a list of (move, weight).
    ValueError for an unknown object, more than MAX_MOVES moves, an empty list or a weight that is not finite and > 0."""
    if isinstance(moves, MoveSet):
        return moves
    if isinstance(moves, (StretchMove, DEMove)):
        return MoveSet([moves], [1.0])
    try:
        items = list(moves)
    except TypeError:
        raise ValueError('moves: a move, a list of moves or a list of (move, weight); got {!r}'.format(moves)) from None
    if not items:
        raise ValueError('moves: the list is empty')
    if len(items) > MAX_MOVES:
        raise ValueError('moves: a set holds at most {} moves ({} given)'.format(MAX_MOVES, len(items)))
    ms, ws = [], []
    for it in items:
        if isinstance(it, (tuple, list)):
            if len(it) != 2:
                raise ValueError('moves: entries are moves or (move, weight) pairs; got {!r}'.format(it))
            mv, w = it
        else:
            mv, w = it, 1.0
        if not isinstance(mv, (StretchMove, DEMove)):
            raise ValueError('moves: {!r} is not a StretchMove or a DEMove'.format(mv))
        try:
            w = float(w)
        except (TypeError, ValueError):
            raise ValueError('moves: the weight {!r} is not a number'.format(w)) from None
        if not (np.isfinite(w) and w > 0.0):
            raise ValueError('moves: weights must be finite and > 0 (got {})'.format(w))
        ms.append(mv)
        ws.append(w)
    return MoveSet(ms, ws)


# ---- the general layout from uniforms: shared by the host generators and the counter restatement ------------------------
def choose_kind(mset, u):
    """The move of each iteration: the first i with u < cumulative weight (the last one if rounding leaves none)."""
    i = np.minimum(np.searchsorted(mset.cum, np.asarray(u), side='right'), len(mset) - 1)
    return i.astype(np.int32)


def de_pair(u, nc):
    """An ordered pair of two DISTINCT indices below nc from one uniform, uniform over the nc (nc - 1) ordered pairs."""
    npairs = nc * (nc - 1)
    p = np.minimum(np.floor(u * float(npairs)).astype(np.int64), npairs - 1)
    j1 = p // (nc - 1)
    r = p % (nc - 1)
    j2 = r + (r >= j1)
    return j1.astype(np.int32), j2.astype(np.int32)


def normal_deviate(u1, u2):
    """Box-Muller: sqrt(-2 ln(1 - u1)) cos(2 pi u2)."""
    return np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(6.283185307179586 * u2)


def general_draws(mset, ndim, ns, which, uz, up, ua, ud, u1, u2):
    """(kind, p1, p2, g, fac, logu) of m iterations from their uniforms.  ``which`` (m,): the index in the set of each
    iteration's move; uz, up, ua (m, 2, ns): the stretch factor's, the partner's and the accept draw's uniforms; ud, u1,
    u2 (m, 2, ns) or None for a set without a DE move: the pair's and the two Box-Muller uniforms."""
    m = len(which)
    kinds = np.asarray(mset.kinds, dtype=np.int32)
    kind = kinds[which]
    p1 = np.empty((m, 2, ns), dtype=np.int32)
    p2 = np.empty((m, 2, ns), dtype=np.int32)
    g = np.empty((m, 2, ns))
    fac = np.empty((m, 2, ns))
    with np.errstate(divide='ignore'):
        logu = np.log(ua)
    for i, mv in enumerate(mset.moves):
        rows = np.nonzero(which == i)[0]
        if not len(rows):
            continue
        if mv.kind == MOVE_STRETCH:
            t1 = (mv.a - 1.0) * uz[rows] + 1.0
            zz = (t1 * t1) / mv.a
            part = np.minimum((up[rows] * ns).astype(np.int32), ns - 1)
            p1[rows], p2[rows], g[rows] = part, part, zz
            fac[rows] = (float(ndim) - 1.0) * np.log(zz)
        else:
            j1, j2 = de_pair(ud[rows], ns)
            t = mv.sigma * normal_deviate(u1[rows], u2[rows])
            p1[rows], p2[rows] = j1, j2
            g[rows] = mset.gamma0(i, ndim) * (1.0 + t)
            fac[rows] = 0.0
    return kind, p1, p2, g, fac, logu


def counter_draws_moves(seed, mset, ndim, first_iter, m, nwalkers):
    """NumPy restatement of the DEVICE generator for a set of moves (csrc/move_kernels.h, moves_draw_kernel): the general
    layout of iterations ``first_iter .. first_iter + m - 1`` keyed by ``seed``.  The split (stream 0) and u_z, u_p, u_a
    (streams 1..6) are ``sampler.counter_draws``'s; stream 7, index 0 is the iteration's move choice; per half-step h,
    stream 8 + 3h is the DE pair and 9 + 3h, 10 + 3h the two Box-Muller uniforms.  Integers equal the device's bit for
    bit; the logarithms and the cosine go through NumPy's (last-place differences)."""
    from .sampler import counter_streams
    mset = parse_moves(mset)
    nw, ns = int(nwalkers), int(nwalkers) // 2
    sidx, cidx, uniform = counter_streams(seed, first_iter, m, nw)
    uz, up, ua = (np.stack([uniform(k + 3 * h, ns) for h in (0, 1)], axis=1) for k in (1, 2, 3))
    which = choose_kind(mset, uniform(7, 1)[:, 0])
    ud, u1, u2 = (np.stack([uniform(k + 3 * h, ns) for h in (0, 1)], axis=1) for k in (8, 9, 10))
    return (sidx, cidx) + general_draws(mset, ndim, ns, which, uz, up, ua, ud, u1, u2)
