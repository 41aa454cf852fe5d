"""Parallel tempering: a ladder of ensembles, each sampling ``ln prior(x) + beta_t ln L(x)``.

``1 = beta_0 > beta_1 > ... > beta_{T-1} > 0``; rung 0 is the posterior, the hot rungs cross between modes that differ in
width or orientation and hand their walkers down.  Per ABSOLUTE iteration i every rung t takes one iteration of the general
layout (``mcmc_spec_amd.moves``: the split, the iteration's move, the proposals, ``fac`` and ``ln u`` of a member of ``nw``
walkers keyed by ``seeds[t]``) with the accept rule

    ln u < (fac + P_t(q)) - P_t(s),     P_t(x) = lpr(x) + beta_t * ll(x)     (two roundings; P_t(s) from the stored lpr, ll)

and then the swap sweep runs, for t = T-1 down to 1 and every walker index w independently: walker w of rung t and walker
w of rung t-1 exchange coordinates, ``ll`` and ``lpr`` when ``ln u < (beta[t-1] - beta[t]) * (ll[t][w] - ll[t-1][w])`` (a
NaN compares false).  The sweep is serial in t, so a walker can travel several rungs in one iteration.  The chain row of
iteration i is the state AFTER the sweep.  ``TemperedSampler`` is this text as a host loop -- the definition;
``DeviceTemperedSampler`` keeps the ladder resident on the GPU (``msx_tempered_*``) and walks the same chain bit for bit.

The swap draws: device-drawn, ``u = counter_uniform(seeds[0], i, 14, (t-1) * 4096 + w)`` (stream 14 of the counter
generator; ``counter_swap_logu`` restates it); host-drawn, ``swap_generator(seeds[0])``, one float64 ``ln u`` per
(iteration, pair, walker), consumed row by row.

What a finished ladder gives.  Rungs are members: ``get_autocorr_time(t)``, ``get_summary(t)`` and
``get_products(cols, t)`` are the other samplers' (sections 12, 14, 15) for rung t -- ``t=None`` for every rung -- and
``DeviceTemperedSampler(autocorr='device')`` keeps the rows in two device series while the run goes
(``msx_series_attach_tempered``), so none of them downloads or uploads a chain.  And the evidence: with ``m_t`` the mean
of ``ln L`` over rung t's stored samples (``mean_log_like``), ``log_evidence`` estimates ``ln Z = int_0^1 <ln L>_beta dbeta``

  * ``method='ti'`` (thermodynamic integration; Lartillot & Philippe 2006): the trapezoid over the ladder,
    ``ln Z = sum_p (beta_p - beta_{p+1}) (m_p + m_{p+1}) / 2  +  beta_{T-1} m_{T-1}``;
  * ``method='ss'`` (the stepping stone; Xie et al. 2011): ``ln Z = sum_{t >= 1} lme_t  +  beta_{T-1} m_{T-1}`` with
    ``lme_t = ln mean exp((beta_{t-1} - beta_t) ln L)`` over rung t's samples, computed around their maximum.

The last term of both is ptemcee's convention for a ladder that stops above beta = 0: the hottest rung's mean continued
to 0, a rectangle.  BOTH ESTIMATES OMIT [0, beta_min] EXCEPT FOR THAT RECTANGLE: ``<ln L>_beta`` usually falls steeply
there (for a d-dimensional Gaussian likelihood as ``-d / (2 beta)``), so an evidence run wants a much smaller ``beta_min``
than a mode-hopping run -- small enough that the hottest rung samples the prior.  ``mc_error`` is the standard error of
the estimates of ``blocks`` consecutive blocks of the stored rows, ``sqrt(var(ddof=1) / blocks)`` (NaN for one block; it
knows nothing of a burn-in left in, and underestimates when a block is shorter than the autocorrelation time);
``ladder_error`` is ``|ln Z - ln Z(rungs [::2], the last rung kept)|``, the estimate's change when every other rung is
dropped.  ``TemperedSampler``'s NumPy (``host_evidence``) is the definition; the device computes the same sums in a fixed
order of its own (``msx_series_evidence``; tests/evidence_numpy.py restates that order).

Adaptive ladders.  ``adaptive=True`` on either sampler: iteration i is the iteration above on the
CURRENT ladder (``db`` formed from it), and after its sweep ``ladder_step`` moves the rungs between the two pinned ends with
the swaps this iteration accepted -- the temperature dynamics of Vousden, Farr & Mandel (2016), renormalised onto the
ladder's span -- until adjacent pairs swap at equal rates.  ``adaptation_lag`` and ``adaptation_time`` are ptemcee's; the
step decays as ``lag / (k + lag)`` with k = ``_adapted``, the adaptive iterations done, which ``reset()`` leaves alone.
``run_mcmc(state, n, adapt=False)`` is the freeze call for the production run.  ``betas`` is the ladder after the last
iteration, ``get_betas()`` the ladder each stored iteration ran WITH, ``ladder_skipped`` the steps dropped because two rungs
would have met.  ``log_evidence`` refuses rows of a moving ladder.  ``ladder_step`` and ``ladder_exp`` are float64
``+ - * /`` only: the host loop, msx_ladder_step and the device's tempered_adapt_kernel give the same bits.

Every target's ladder in one run.  ``GroupTemperedSampler`` steps K ``TemperedSampler``s in lock-step,
two batched evaluations per half-step for all targets -- the definition; ``DeviceGroupTemperedSampler`` keeps the K x T rungs
of a ``TargetGroup`` resident as the members of ONE ensemble (``msx_group_tempered_*``: eight launches per iteration for all
targets) and target k walks, bit for bit, the chain of its own ladder run alone.  ``sampler.target(k)`` is target k's ladder
with everything above.
"""
from __future__ import annotations

from collections import namedtuple
from contextlib import closing

import numpy as np

from .sampler import EnsembleSampler, State, _propose, _pump, device_seed
from .stored import StoredChain

MAX_TEMPS = 64        # include/msx.h MSX_MAX_GROUP: rungs of a ladder
SWAP_STREAM = 14      # the counter generator's stream of the swap draws (0..13: moves.counter_draws_moves)
SWAP_STRIDE = 4096    # index = (t - 1) * SWAP_STRIDE + w: at most 64 rungs of at most 4,096 walkers, below 2^24
W_REJECT = 1          # include/msx.h MSX_W_REJECT


def default_betas(ntemps, beta_min):
    """A geometric ladder from 1 down to ``beta_min``."""
    return np.geomspace(1.0, float(beta_min), int(ntemps))


def resolve_betas(ntemps, betas, beta_min=0.02):
    """The ladder of ``ntemps`` rungs (``default_betas(ntemps, beta_min)``) or the given ``betas``, checked: 1..64 rungs,
    finite, > 0, strictly descending; both given must agree in length.  ValueError otherwise."""
    if betas is None:
        if ntemps is None:
            raise ValueError('give ntemps or betas')
        if not 1 <= int(ntemps) <= MAX_TEMPS:
            raise ValueError('a ladder has 1..{} rungs ({} asked for)'.format(MAX_TEMPS, ntemps))
        betas = default_betas(ntemps, beta_min) if int(ntemps) > 1 else np.array([1.0])
    b = np.array(betas, dtype=np.float64).reshape(-1)
    if ntemps is not None and int(ntemps) != len(b):
        raise ValueError('ntemps = {} but {} betas given'.format(ntemps, len(b)))
    if not 1 <= len(b) <= MAX_TEMPS:
        raise ValueError('a ladder has 1..{} rungs ({} given)'.format(MAX_TEMPS, len(b)))
    if not np.all(np.isfinite(b)) or np.any(b <= 0.0):
        raise ValueError('betas must be finite and > 0')
    if np.any(np.diff(b) >= 0.0):
        raise ValueError('betas must be strictly descending')
    return b


_EXP_COEF = [1.0]
for _k in range(1, 13):
    _EXP_COEF.append(_EXP_COEF[-1] * _k)        # k! (exact in float64)
_EXP_COEF = [1.0 / f for f in _EXP_COEF]        # c[k] = 1.0 / k!


def ladder_exp(x):
    """The adaptive ladder's exponential for |x| <= 1, in float64 ``+ * /`` only, so NumPy, host C and
    the device give the same bits: ``y = x * 0.125``, the degree-12 Taylor polynomial in y by Horner from the top, squared
    three times.  Within 7 ulp of ``np.exp`` on [-1, 1]; exactly 1.0 at 0.  A scalar or an array."""
    y = np.asarray(x, dtype=np.float64) * 0.125
    p = np.full(y.shape, _EXP_COEF[12])
    for k in range(11, -1, -1):
        p = p * y
        p = p + _EXP_COEF[k]
    for _ in range(3):
        p = p * p
    return p if p.ndim else float(p)


def check_adaptation(lag, time):
    """(lag, time) as floats; ValueError unless lag is finite and > 0 and time is finite and >= 1 (which keeps |dS| <= 1)."""
    lag, time = float(lag), float(time)
    if not np.isfinite(lag) or lag <= 0.0:
        raise ValueError('adaptation_lag must be finite and > 0')
    if not np.isfinite(time) or time < 1.0:
        raise ValueError('adaptation_time must be finite and >= 1')
    return lag, time


def ladder_step(betas, counts, nw, k, lag, time):
    """One step of the temperature dynamics (Vousden, Farr & Mandel 2016): ``(betas', skipped)``.

    ``betas`` (T,) strictly descending; ``counts`` (T-1,) the swaps accepted in THIS iteration, pair p = rungs (p + 1, p);
    ``k`` the adaptive iterations done before this one.  With ``r = counts / nw``, ``kappa = (lag / (k + lag)) / time`` and
    ``Ti = 1 / betas``, the gap ``g[p] = Ti[p] - Ti[p-1]`` of every free rung p = 1..T-2 is scaled by
    ``ladder_exp(kappa * (r[p-1] - r[p]))`` -- the hottest gap is kept -- and the running sum c of the gaps is renormalised
    onto the ladder's span: ``betas'[p] = 1 / (Ti[0] + (Ti[T-1] - Ti[0]) * (c[p] / c[T-1]))``.  Both ends are the input's.
    T <= 2: unchanged.  A result that is not finite or not strictly descending: the input, and skipped = 1.  float64
    ``+ - * /`` in this order; msx_ladder_step and tempered_adapt_kernel reproduce the bits."""
    lag, time = check_adaptation(lag, time)
    b = np.array(betas, dtype=np.float64).reshape(-1)
    T = len(b)
    if T <= 2:
        return b, 0
    r = np.asarray(counts, dtype=np.float64).reshape(-1) / float(nw)
    if r.shape != (T - 1,):
        raise ValueError('counts: one per adjacent pair')
    decay = lag / (float(k) + lag)
    kappa = decay / time
    Ti = 1.0 / b
    g = np.empty(T)
    g[0] = 0.0
    g[1:] = Ti[1:] - Ti[:-1]
    dS = kappa * (r[:-1] - r[1:])                 # dS[p - 1] for p = 1..T-2
    g[1:T - 1] = g[1:T - 1] * ladder_exp(dS)
    c = np.empty(T)
    c[0] = 0.0
    c[1] = g[1]
    for p in range(2, T):                         # in index order
        c[p] = c[p - 1] + g[p]
    span = Ti[T - 1] - Ti[0]
    out = b.copy()
    with np.errstate(all='ignore'):
        out[1:T - 1] = 1.0 / (Ti[0] + span * (c[1:T - 1] / c[T - 1]))
    if not np.all(np.isfinite(out)) or np.any(out[1:] >= out[:-1]):
        return b, 1
    return out, 0


def resolve_seeds(ntemps, seed, seeds):
    """One 64-bit key per rung: ``seeds``, or ``(device_seed(seed) + t) mod 2^64``."""
    if seeds is not None:
        out = [device_seed(s) for s in seeds]
        if len(out) != ntemps:
            raise ValueError('seeds: one per rung ({} given for {} rungs)'.format(len(out), ntemps))
        return out
    s0 = device_seed(seed)
    return [(s0 + t) & 0xffffffffffffffff for t in range(ntemps)]


def swap_generator(seed0):
    """The host-drawn swap stream of a ladder whose rung 0 is keyed by ``seed0``: one uniform per (iteration, pair, walker),
    row by row -- m iterations at once are m calls of one.  Defined here once, for both samplers."""
    return np.random.Generator(np.random.PCG64(np.random.SeedSequence(int(seed0), spawn_key=(SWAP_STREAM,))))


def draw_swap_logu(rng, m, ntemps, nwalkers):
    """``ln u`` (m, ntemps - 1, nwalkers) of m iterations from the swap stream; row p belongs to the pair (p + 1, p)."""
    u = rng.random((int(m), int(ntemps) - 1, int(nwalkers)))
    with np.errstate(divide='ignore'):
        return np.log(u)


def counter_swap_logu(seed0, first_iter, m, ntemps, nwalkers):
    """NumPy restatement of the DEVICE's swap draws (csrc/tempered_kernels.h, tempered_swap_draw_kernel): ``ln u`` (m,
    ntemps - 1, nwalkers) of iterations ``first_iter ..`` -- stream 14, index ``(t - 1) * 4096 + w`` for the pair (t, t - 1).
    The uniforms equal the device's bit for bit; the logarithm goes through NumPy's (last-place differences)."""
    from .sampler import counter_streams
    T, nw = int(ntemps), int(nwalkers)
    if T < 2:
        return np.empty((int(m), 0, nw))
    _, _, uniform = counter_streams(seed0, first_iter, m, 2)
    u = uniform(SWAP_STREAM, (T - 2) * SWAP_STRIDE + nw)
    cols = (np.arange(T - 1)[:, None] * SWAP_STRIDE + np.arange(nw)[None, :]).ravel()
    with np.errstate(divide='ignore'):
        return np.log(np.ascontiguousarray(u[:, cols])).reshape(int(m), T - 1, nw)


def counter_draws_tempered(seeds, mset, ndim, first_iter, m, nwalkers):
    """NumPy restatement of ``ctx.tempered_draw``: ``(members, swap_logu)`` of iterations ``first_iter .. first_iter + m - 1``
    -- rung t is ``moves.counter_draws_moves(seeds[t], ...)`` unchanged (streams 0..13), the swap draws are stream 14 of
    ``seeds[0]``."""
    from .moves import counter_draws_moves
    members = [counter_draws_moves(s, mset, ndim, first_iter, m, nwalkers) for s in seeds]
    return members, counter_swap_logu(seeds[0], first_iter, m, len(seeds), nwalkers)


def _values(out):
    """(values, statuses or None) of what a density function returned: an array, or ``(values, statuses)``."""
    if isinstance(out, tuple):
        return np.asarray(out[0], dtype=float), np.asarray(out[1])
    return np.asarray(out, dtype=float), None


def _accept_rung(beta, coords, ll, lpr, accepted, draws, h, q, lpr_q, ll_q):
    """The accept rule of half h of one rung, in place."""
    s_idx, fac, logu = draws[0][0, h], draws[-2][0, h], draws[-1][0, h]
    with np.errstate(invalid='ignore'):   # -inf - -inf = nan -> compares False -> rejected
        prod_q = beta * ll_q
        p_q = lpr_q + prod_q
        prod_s = beta * ll[s_idx]
        p_s = lpr[s_idx] + prod_s
        lnpdiff = (fac + p_q) - p_s
    acc = logu < lnpdiff
    coords[s_idx[acc]] = q[acc]
    ll[s_idx[acc]] = ll_q[acc]
    lpr[s_idx[acc]] = lpr_q[acc]
    accepted[s_idx[acc]] = True


def swap_sweep(db, coords, ll, lpr, swap_logu, nswap):
    """The sweep of one iteration, in place on coords (T, nw, ndim), ll, lpr (T, nw); swap_logu (T-1, nw); nswap (T-1,)
    counts the swaps accepted per pair.  db[p] = beta[p] - beta[p + 1]."""
    for t in range(len(ll) - 1, 0, -1):
        with np.errstate(invalid='ignore'):
            d = ll[t] - ll[t - 1]
            lnr = db[t - 1] * d
        sw = swap_logu[t - 1] < lnr
        for arr in (coords, ll, lpr):
            tmp = arr[t, sw].copy()
            arr[t, sw] = arr[t - 1, sw]
            arr[t - 1, sw] = tmp
        nswap[t - 1] += int(np.count_nonzero(sw))


LogEvidence = namedtuple('LogEvidence', ['log_z', 'mc_error', 'ladder_error', 'mean_log_like'])
MAX_BLOCKS = 64       # csrc/evidence_kernels.h kEvdMaxBlocks


def block_bounds(n, blocks):
    """The ``blocks`` consecutive blocks of n rows: block b is rows ``lo[b] .. lo[b + 1] - 1``, ``lo[b] = floor(b n / blocks)``."""
    n, blocks = int(n), int(blocks)
    if not 1 <= blocks <= min(n, MAX_BLOCKS):
        raise ValueError("blocks must lie in 1 .. min(n', {})".format(MAX_BLOCKS))
    return [b * n // blocks for b in range(blocks + 1)]


def _lme(x, db):
    """``ln mean exp(db x)`` of a flat sample around its maximum; -inf values weigh zero, all -inf gives -inf."""
    M = np.max(x)
    if np.isnan(M):
        return np.nan
    if M == -np.inf:
        return -np.inf
    with np.errstate(invalid='ignore'):
        e = np.where(x == -np.inf, 0.0, np.exp(db * (x - M)))
    return db * M + np.log(np.sum(e) / x.size)


def host_evidence(x, db=None, blocks=1):
    """(mean, lme), each (T, blocks + 1), of x (n', T, nw): [:, 0] over all rows and walkers of a member, [:, 1 + b] over
    block b's rows (``block_bounds``); lme = ``ln mean exp(db[t] x)`` (None without db).  What msx_series_evidence computes,
    in NumPy's summation order."""
    x = np.asarray(x, dtype=float)
    lo = block_bounds(x.shape[0], blocks)
    T = x.shape[1]
    parts = [x] + [x[lo[b]:lo[b + 1]] for b in range(int(blocks))]
    with np.errstate(invalid='ignore'):
        mean = np.array([[np.mean(p[:, t]) for p in parts] for t in range(T)])
    if db is None:
        return mean, None
    return mean, np.array([[_lme(p[:, t].ravel(), db[t]) for p in parts] for t in range(T)])


def ti_log_z(betas, m):
    """The trapezoid of the rung means m over the ladder, plus ``beta_{T-1} m_{T-1}`` (the module docstring)."""
    betas, m = np.asarray(betas, dtype=float), np.asarray(m, dtype=float)
    return float(np.sum((betas[:-1] - betas[1:]) * (m[:-1] + m[1:]) / 2.0) + betas[-1] * m[-1])


def ss_log_z(betas, lme, m_last):
    """The stepping stone: ``sum_{t >= 1} lme[t] + beta_{T-1} m_last`` (lme[0] is not used)."""
    return float(np.sum(np.asarray(lme, dtype=float)[1:]) + np.asarray(betas, dtype=float)[-1] * m_last)


def halved(ntemps):
    """The rungs [::2] with the last one kept."""
    idx = list(range(0, int(ntemps), 2))
    return idx if idx[-1] == int(ntemps) - 1 else idx + [int(ntemps) - 1]


def _ss_db(betas, idx):
    """db (T,) of the stepping stone over the rungs idx: member idx[j] gets ``beta[idx[j-1]] - beta[idx[j]]``, the others 0."""
    db = np.zeros(len(betas))
    for a, b in zip(idx[:-1], idx[1:]):
        db[b] = betas[a] - betas[b]
    return db


class _Ladder:
    """What both samplers keep and return."""

    _series = _dens = None   # DeviceTemperedSampler(autocorr='device'): the chain's and the densities' device series
    engine = None            # the staged Engine, where the sampler was built on one (get_summary, get_products)
    _device_modes = False    # get_modes: the device calls (the device samplers) or the definition (TemperedSampler)

    def _flat_members(self, members=None):
        """The stored chain as (n, T nw, ndim): the rungs as members, side by side; ``members``: those rungs alone."""
        if not self._chain:
            raise ValueError('the selection rows[0:n][discard::thin] is empty')
        x = np.array(self._chain) if members is None else np.array(self._chain)[:, list(members)]
        return x.reshape(len(self._chain), -1, self.ndim)

    def _stored(self):
        """The view of the stored chain that the analyses below ask (mcmc_spec_amd.stored): the rungs
        are its members."""
        T = self.ntemps
        return StoredChain(self._series, self._flat_members, len(self._chain), self.ndim, [self.nwalkers] * T,
                           None if self.engine is None else [self.engine] * T, device_modes=self._device_modes, joined=True)

    def get_autocorr_time(self, t=0, quiet=False, c=5.0, tol=50.0, discard=0, thin=1):
        """Rung t's integrated autocorrelation time (ndim,) -- rung 0 is the posterior -- or every rung's (T, ndim) for
        ``t=None``: ``EnsembleSampler.get_autocorr_time``'s rules and keywords.  With autocorr='device' from the chain on
        the device, one msx_series_acf call per lag tile over all rungs."""
        return self._stored().autocorr_time(t, quiet, c, tol, discard, thin)

    def get_rhat(self, t=0, discard=0, thin=1, cols=None):
        """Rung t's split R-hat (ncols,) over its walkers -- rung 0 is the posterior -- or every rung's (T, ncols) for
        ``t=None`` (``EnsembleSampler.get_rhat``'s keywords and rules).  From the device series with
        autocorr='device' (one msx_series_moments call over all members), otherwise ``diagnostics`` on the host chain."""
        return self._stored().moments(t, discard, thin, cols, False)['rhat']

    def get_moments(self, t=0, discard=0, thin=1, cols=None):
        """Rung t's {'mean', 'cov', 'count'} (``EnsembleSampler.get_moments``); ``t=None``: every rung's."""
        out = self._stored().moments(t, discard, thin, cols, rhat=False)
        return {name: out[name] for name in ('mean', 'cov', 'count')}

    def get_rank_rhat(self, t=0, discard=0, thin=1, cols=None):
        """Rung t's {'bulk', 'folded', 'rhat'} -- rung 0 is the posterior -- or every rung's for ``t=None``
        (``EnsembleSampler.get_rank_rhat``): from the device series with autocorr='device', otherwise
        ``diagnostics`` on the host chain."""
        return self._stored().rank_rhat(t, discard, thin, cols)

    def get_ess(self, t=0, discard=0, thin=1, cols=None, kind='bulk'):
        """Rung t's effective sample size (ncols,), or every rung's (T, ncols) for ``t=None`` (``EnsembleSampler.get_ess``)."""
        return self._stored().ess(t, discard, thin, cols, kind)

    def get_mcse(self, t=0, discard=0, thin=1, cols=None, q=(0.16, 0.5, 0.84)):
        """Rung t's {'mean', 'quantiles'}, or every rung's for ``t=None`` (``EnsembleSampler.get_mcse``)."""
        return self._stored().mcse(t, discard, thin, cols, q)

    def get_modes(self, t=0, ncomp=2, discard=0, thin=1, cols=None, **fit_kw):
        """Rung t's posterior modes -- rung 0 is the posterior -- as ``EnsembleSampler.get_modes`` gives them (a
        ``modes.ModeFit`` cut to that rung); ``t=None``: every rung's, one member per rung.  TemperedSampler uses the
        definition on the host chain; the device samplers the chain held on the device with autocorr='device' (every rung's
        jobs in one msx_series_modes call) and upload the host chain otherwise."""
        return self._stored().modes(t, ncomp, discard, thin, cols, **fit_kw)

    def get_summary(self, t=0, q=(0.16, 0.5, 0.84), discard=0, thin=1, cols=None):
        """Rung t's posterior summary over its stored chain, flattened over its walkers (``DeviceEnsembleSampler.get_summary``'s
        dict and numbers: DESIGN.md section 14); ``t=None``: every rung's, the arrays with a leading axis T.  With
        autocorr='device' from the chain held there; otherwise the host chain is uploaded first (the sampler must have
        been built on an Engine)."""
        return self._stored().summary(t, q, discard, thin, cols)

    def get_products(self, cols, t=0, q=(0.16, 0.5, 0.84), discard=0, thin=1, indices=None):
        """``get_summary``'s dict over DERIVED columns (``mcmc_spec_amd.products``) of rung t's stored chain (``t=None``: every
        rung's), as ``DeviceEnsembleSampler.get_products``; the one engine serves every rung.
        ``indices``: positions in the rung's flat sample ``get_chain(t, discard=, thin=, flat=True)`` to use instead of all
        of it; those go through msx_products_batch from the host copy."""
        return self._stored().products(cols, t, q, discard, thin, indices)

    def get_predictive(self, t=0, q=(0.16, 0.5, 0.84), discard=0, thin=1):
        """Rung t's posterior predictive check (``mcmc_spec_amd.predictive``) of its stored chain --
        rung 0 is the posterior --, ``predictive.check``'s dict (``worst_status`` in place of ``terms`` and ``status``);
        ``t=None``: a list of every rung's.  With autocorr='device' from the chain held there, otherwise the host chain is
        uploaded first (the sampler must have been built on an Engine with staged products)."""
        return self._stored().predictive(t, q, discard, thin)

    def get_loo(self, t=0, discard=0, thin=1, reff=1.0):
        """Rung t's PSIS-LOO, WAIC and khat per observation (``mcmc_spec_amd.psis``) of its stored
        chain -- rung 0 is the posterior --, ``psis.loo``'s dict; ``t=None``: a list of every rung's.  With autocorr='device'
        from the chain held there, otherwise the host chain is uploaded first."""
        return self._stored().loo(t, discard, thin, reff)

    def get_reweighted(self, engines_new=None, t=0, mode='logposterior', discard=0, thin=1):
        """What rung t's stored chain says about another density (``mcmc_spec_amd.reweight``): a
        ``reweight.Reweighted`` of one member whose log-weight is ``lp_new - lpr - betas[t] * ll`` -- ``lp_new`` the
        ``mode`` of ``engines_new`` (one staged Engine; None: this sampler's own, and the weights are then those of the
        rung against the posterior, ``(1 - beta) * ll``), ``lpr`` and ``ll`` the chain scored once more under the sampler's
        own engine.  With autocorr='device' on the chain held there; otherwise the host chain is uploaded first.  The
        selected rows must all have been run with the ladder ``self.betas``."""
        view = self._stored()
        view._need_gpu()
        if np.any(self.get_betas(discard=discard, thin=thin) != self.betas):
            raise ValueError('get_reweighted: the selected rows were not all run with the ladder self.betas (an adaptive run moved it): '
                             'freeze the ladder (adapt=False) and discard= the adaptive rows')
        return view.reweighted([self.engine if engines_new is None else engines_new] * self.ntemps, int(t), self.betas, mode=mode,
                               discard=discard, thin=thin)

    def _evidence(self, discard, thin, db, blocks):
        """(mean, lme) (T, blocks + 1) of the stored ln L: ``host_evidence``, or msx_series_evidence on the device series (this
        ladder's db scattered to its rungs among the series' members)."""
        view = self._stored()
        view._need(discard, thin, 1)
        if self._dens is None:
            return host_evidence(np.array(self._ll)[int(discard)::int(thin)], db, blocks)
        if db is not None:
            full = np.zeros(self._dens.k)
            full[view.own] = db
            db = full
        mean, lme = self._dens.evidence(view.n, discard, thin, 0, db, blocks)
        return mean[view.own], None if lme is None else lme[view.own]

    def mean_log_like(self, discard=0, thin=1):
        """(T,): the mean of ``ln L`` over each rung's stored samples, ``<ln L>_beta`` at the ladder's betas."""
        return self._evidence(discard, thin, None, 1)[0][:, 0].copy()

    def log_evidence(self, discard=0, thin=1, blocks=8, method='ti'):
        """``LogEvidence(log_z, mc_error, ladder_error, mean_log_like)`` of the stored run (the module docstring):
        ``method='ti'`` thermodynamic integration, ``'ss'`` the stepping stone; ``blocks`` consecutive blocks of the rows for
        ``mc_error`` (1 .. min(rows, 64))."""
        if method not in ('ti', 'ss'):
            raise ValueError("method must be 'ti' or 'ss'")
        T, betas, blocks = self.ntemps, self.betas, int(blocks)
        if np.any(self.get_betas(discard=discard, thin=thin) != betas):
            raise ValueError('log_evidence: the selected rows were not all run with the ladder self.betas (an adaptive run moved it): '
                             'freeze the ladder (adapt=False) and discard= the adaptive rows')
        half = halved(T)
        if method == 'ti':
            mean, _ = self._evidence(discard, thin, None, blocks)
            est = np.array([ti_log_z(betas, mean[:, j]) for j in range(blocks + 1)])
            coarse = ti_log_z(betas[half], mean[half, 0])
        else:
            mean, lme = self._evidence(discard, thin, _ss_db(betas, list(range(T))), blocks)
            est = np.array([ss_log_z(betas, lme[:, j], mean[-1, j]) for j in range(blocks + 1)])
            lme2 = self._evidence(discard, thin, _ss_db(betas, half), 1)[1]
            coarse = ss_log_z(betas[half], lme2[half, 0], mean[-1, 0])
        with np.errstate(invalid='ignore'):
            mc = float(np.sqrt(np.var(est[1:], ddof=1) / blocks)) if blocks > 1 else float('nan')
            ladder = float(abs(est[0] - coarse))
        return LogEvidence(float(est[0]), mc, ladder, mean[:, 0].copy())

    def _init_ladder(self, nwalkers, ndim, ntemps, betas, beta_min, seed, seeds, moves, adaptive=False, adaptation_lag=10000.0,
                     adaptation_time=100.0):
        self.betas = resolve_betas(ntemps, betas, beta_min)   # the ladder after the last iteration (never changed in place)
        self.ntemps = len(self.betas)
        self.adaptive = bool(adaptive)
        self.adaptation_lag, self.adaptation_time = check_adaptation(adaptation_lag, adaptation_time)
        self._adapted = 0          # k: adaptive iterations done (on the device: queued); reset() leaves it alone, as _drawn
        self.ladder_skipped = 0    # ladder steps that would have collapsed the ladder and were skipped
        self.nwalkers, self.ndim = int(nwalkers), int(ndim)
        if self.nwalkers % 2 or self.nwalkers < 2:
            raise ValueError('a rung needs an even number of walkers')
        self.seeds = resolve_seeds(self.ntemps, seed, seeds)
        from .moves import StretchMove
        # every rung is a member in the general layout; its generators are EnsembleSampler's for seeds[t]
        self._rungs = [EnsembleSampler(self.nwalkers, self.ndim, None, seed=s, moves=StretchMove() if moves is None else moves,
                                       _general=True) for s in self.seeds]
        self._moves = self._rungs[0]._moves
        self._swap_rng = swap_generator(self.seeds[0])
        self._drawn = 0
        self.reset()

    def reset(self):
        """Forget the stored chain and counts.  The streams' positions (and ``_drawn``) are left alone."""
        self._chain, self._ll, self._lpr, self._betas_rows = [], [], [], []
        self._accepted = np.zeros((self.ntemps, self.nwalkers))
        self._nswap = np.zeros(max(self.ntemps - 1, 0), dtype=np.int64)
        self.iteration = 0
        self._last = None

    def _rows(self, rows, t, flat, thin, discard, tail):
        a = np.array(rows)[discard::thin] if rows else np.empty((0, self.ntemps, self.nwalkers) + tail)
        if t is not None:
            a = a[:, int(t)]
            return a.reshape((-1,) + tail) if flat else a
        return np.moveaxis(a, 1, 0).reshape((self.ntemps, -1) + tail) if flat else a

    def get_chain(self, t=0, flat=False, thin=1, discard=0):
        """Rung t's chain (steps, nw, ndim) -- rung 0 is the posterior; ``t=None``: all rungs, (steps, T, nw, ndim).  flat:
        the steps and walkers merged."""
        return self._rows(self._chain, t, flat, thin, discard, (self.ndim,))

    def get_betas(self, discard=0, thin=1):
        """(steps, T): the ladder each stored iteration was run WITH (constant rows unless the run was adaptive)."""
        return np.array(self._betas_rows, dtype=np.float64).reshape(-1, self.ntemps)[discard::thin]

    def _adapting(self, adapt):
        return self.adaptive if adapt is None else bool(adapt)

    def get_log_like(self, t=0, flat=False, thin=1, discard=0):
        return self._rows(self._ll, t, flat, thin, discard, ())

    def get_log_prior(self, t=0, flat=False, thin=1, discard=0):
        return self._rows(self._lpr, t, flat, thin, discard, ())

    def get_log_prob(self, t=0, flat=False, thin=1, discard=0):
        """``lpr + ll``: the untempered posterior of rung t's samples."""
        return self.get_log_prior(t, flat, thin, discard) + self.get_log_like(t, flat, thin, discard)

    @property
    def acceptance_fraction(self):
        """(T, nw): moves accepted per iteration (swaps are not counted)."""
        return self._accepted / max(self.iteration, 1)

    @property
    def swap_fraction(self):
        """(T-1,): swaps accepted between rungs p + 1 and p / (iterations x nw)."""
        return self._nswap / float(max(self.iteration, 1) * self.nwalkers)

    def get_last_sample(self):
        return self._last

    def run_mcmc(self, initial_state, nsteps, **kw):
        st = None
        for st in self.sample(initial_state, iterations=nsteps, **kw):
            pass
        return st

    def _start(self, initial_state):
        """(coords (T, nw, ndim), ll, lpr (T, nw)) of an initial state: a TemperedState, or coordinates -- (nw, ndim) for
        every rung alike or (T, nw, ndim).  ValueError for a walker outside the prior or with a NaN likelihood."""
        if isinstance(initial_state, TemperedState):
            coords, ll, lpr = (np.array(a, dtype=float) for a in (initial_state.coords, initial_state.log_like, initial_state.log_prior))
        else:
            coords = np.array(initial_state, dtype=float)
            if coords.ndim == 2:
                coords = np.repeat(coords[None], self.ntemps, axis=0)
            ll = lpr = None
        if coords.shape != (self.ntemps, self.nwalkers, self.ndim):
            raise ValueError('incompatible input dimensions')
        if np.any(~np.isfinite(coords)):
            raise ValueError('At least one parameter value was infinite or NaN')
        if ll is None:
            flat = coords.reshape(-1, self.ndim)
            lpr, ll = self._evaluate(flat)
            lpr, ll = lpr.reshape(self.ntemps, -1).copy(), ll.reshape(self.ntemps, -1).copy()
        if not np.all(np.isfinite(lpr)):
            raise ValueError('an initial walker lies outside the prior (its log-prior is not finite)')
        if np.any(np.isnan(ll)):
            raise ValueError('Probability function returned NaN')
        return np.ascontiguousarray(coords), np.ascontiguousarray(ll), np.ascontiguousarray(lpr)


class TemperedState(State):
    """``coords`` (T, nw, ndim), ``log_like``, ``log_prior`` (T, nw); ``log_prob = log_prior + log_like``."""

    def __init__(self, coords, log_like, log_prior):
        self.coords = np.array(coords, dtype=float)
        self.log_like = np.array(log_like, dtype=float)
        self.log_prior = np.array(log_prior, dtype=float)
        self.log_prob = self.log_prior + self.log_like
        self.random_state = None


class TemperedSampler(_Ladder):
    """The host loop, and the definition (the module docstring).  ``loglike_fn`` / ``logprior_fn`` take (n, ndim) and return
    n values, or ``(values, statuses)`` (``ctx.logprob_batch``): a proposal whose prior status is ``MSX_W_REJECT`` is
    rejected whatever its likelihood reports; an error status of the prior, or of the likelihood on a proposal the prior
    admits, raises what ``engine._raise_for_status`` raises.  An ``Engine`` in ``loglike_fn``'s place (``logprior_fn=None``)
    stands for its two status-carrying evaluations.

    ``draws(first_iteration, m)`` (optional) replaces the generators: ``(members, swap_logu)``, members a list of T
    general layouts (m iterations each) and swap_logu (m, T-1, nw) -- ``ctx.tempered_draw`` makes this loop walk the chain
    ``DeviceTemperedSampler(rng='device')`` draws for itself."""

    def __init__(self, nwalkers, ndim, loglike_fn, logprior_fn=None, ntemps=None, betas=None, beta_min=0.02, seed=None, seeds=None,
                 moves=None, draws=None, adaptive=False, adaptation_lag=10000.0, adaptation_time=100.0):
        if logprior_fn is None and hasattr(loglike_fn, 'ctx'):
            from . import _lib
            self.engine = loglike_fn   # (get_summary / get_products upload the host chain to its device)
            ctx = loglike_fn.ctx
            loglike_fn, logprior_fn = (lambda q: ctx.logprob_batch(q, _lib.MODE_LOGLIKE)), (lambda q: ctx.logprob_batch(q, _lib.MODE_LOGPRIOR))
        self.loglike_fn, self.logprior_fn = loglike_fn, logprior_fn
        self._draws = draws
        self._init_ladder(nwalkers, ndim, ntemps, betas, beta_min, seed, seeds, moves, adaptive, adaptation_lag, adaptation_time)

    def _evaluate(self, q):
        """(lpr, ll) of the proposals q with the status rule."""
        from .engine import _raise_for_status
        lpr, st_p = _values(self.logprior_fn(q))
        ll, st_l = _values(self.loglike_fn(q))
        if lpr.shape != (len(q),) or ll.shape != (len(q),):
            raise ValueError('a density function returned the wrong shape')
        if st_p is not None:
            _raise_for_status(st_p, q)
        if st_l is not None:
            admitted = np.isfinite(lpr) if st_p is None else st_p != W_REJECT
            _raise_for_status(np.where(admitted, st_l, 0), q)
        elif np.any(np.isnan(ll) & np.isfinite(lpr)):
            raise ValueError('Probability function returned NaN')
        return lpr, ll

    def _draw_steps(self, m):
        if self._draws is not None:
            out = self._draws(self._drawn, m)
            self._drawn += m
            return out
        return [r._draw_steps(m) for r in self._rungs], draw_swap_logu(self._swap_rng, m, self.ntemps, self.nwalkers)

    def sample(self, initial_state, iterations=1, store=True, adapt=None):
        coords, ll, lpr = self._start(initial_state)
        T, ns = self.ntemps, self.nwalkers // 2
        adapt = self._adapting(adapt)
        for _ in range(int(iterations)):
            members, swap_logu = self._draw_steps(1)
            betas = self.betas
            db = betas[:-1] - betas[1:]                       # in float64, from the ladder of this iteration
            before = self._nswap.copy()
            accepted = np.zeros((T, self.nwalkers), dtype=bool)
            for h in (0, 1):
                q = np.concatenate([_propose(coords[t], members[t], h) for t in range(T)])
                lpr_q, ll_q = self._evaluate(q)
                for t in range(T):
                    sl = slice(t * ns, (t + 1) * ns)
                    _accept_rung(betas[t], coords[t], ll[t], lpr[t], accepted[t], members[t], h, q[sl], lpr_q[sl], ll_q[sl])
            swap_sweep(db, coords, ll, lpr, np.asarray(swap_logu)[0], self._nswap)
            if adapt:
                self.betas, skipped = ladder_step(betas, self._nswap - before, self.nwalkers, self._adapted, self.adaptation_lag,
                                                  self.adaptation_time)
                self._adapted += 1
                self.ladder_skipped += skipped
            self._accepted += accepted
            self.iteration += 1
            if store:
                self._betas_rows.append(betas)
                self._chain.append(coords.copy())
                self._ll.append(ll.copy())
                self._lpr.append(lpr.copy())
            self._last = TemperedState(coords, ll, lpr)
            yield self._last


class DeviceTemperedSampler(_Ladder):
    """The ladder resident on the GPU (``msx_tempered_*``; csrc/tempered_kernels.h): per half-step ONE launch proposes for
    all T rungs, the plain evaluation scores the ``T * nw / 2`` proposals twice (prior, likelihood), and after the second
    half-step one launch sweeps the swaps; only the chains come back.  ``engine`` is a staged ``Engine`` on one GPU.

    ``rng='host'``: the randomness is this object's NumPy generators, exactly ``TemperedSampler``'s calls -- same seed, same
    chain.  ``rng='device'``: the library draws every chunk from ``seeds`` and the ABSOLUTE iteration ``_drawn``, which
    every chunk queued advances and ``reset()`` leaves alone (as ``DeviceEnsembleSampler`` documents: consecutive runs
    continue one stream; a loop left early leaves ``_drawn`` past the last iteration yielded by the chunks already
    queued).  The chain is the one ``TemperedSampler(draws=lambda i, m: ctx.tempered_draw(seeds, moves, i, m, nw, ndim))``
    walks.

    ``adaptive=True`` (the module docstring): the ladder lives on the device (``msx_ladder_adapt``) and a small kernel moves
    it after every sweep.  ``_adapted`` follows ``_drawn``'s rule: it counts the adaptive iterations QUEUED, ``reset()``
    leaves it alone, and after a run ends -- finished or left early -- ``betas`` is the device's ladder behind everything
    queued (``msx_ladder_current``), so the next run, adaptive or frozen, starts from it; while a run goes ``betas`` is still
    the ladder it began with.  A run that does not adapt calls none of the context's ``tempered_adapt`` / ``tempered_betas``
    / ``tempered_ladder``.

    ``autocorr='device'`` (the other device samplers' option): the stored rows are kept on the device as well, in two
    ``_lib.Series`` of T members -- the coordinates, and (ll, lpr) -- that every ``sample(store=True)`` run appends to from
    row ``len(self._chain)`` on (``msx_series_attach_tempered``); ``get_autocorr_time``, ``get_summary``, ``get_products``,
    ``mean_log_like`` and ``log_evidence`` then work there.  ``cap_hint``: the rows to reserve at once (the iterations
    planned, when known); the series grow by doubling otherwise.  ``reset()`` drops the rows.  The chain is the same, bit
    for bit, whatever ``autocorr`` is."""

    _device_modes = True

    def __init__(self, nwalkers, ndim, engine, ntemps=None, betas=None, beta_min=0.02, seed=None, seeds=None, chunk=64, rng='host',
                 moves=None, autocorr='host', cap_hint=0, adaptive=False, adaptation_lag=10000.0, adaptation_time=100.0):
        if rng not in ('host', 'device'):
            raise ValueError("rng must be 'host' or 'device'")
        if autocorr not in ('host', 'device'):
            raise ValueError("autocorr must be 'host' or 'device'")
        self.rng_mode = rng
        self.autocorr = autocorr
        self.engine = engine
        self.chunk = int(chunk)
        self._init_ladder(nwalkers, ndim, ntemps, betas, beta_min, seed, seeds, moves, adaptive, adaptation_lag, adaptation_time)
        if autocorr == 'device':
            from . import _lib
            counts = [self.nwalkers] * self.ntemps
            self._series = _lib.Series(engine.ctx, self.ntemps * self.nwalkers, self.ndim, counts, cap_hint=int(cap_hint))
            self._dens = _lib.Series(engine.ctx, self.ntemps * self.nwalkers, 2, counts, cap_hint=int(cap_hint))

    def _evaluate(self, q):
        from . import _lib
        from .engine import _raise_for_status
        ctx = self.engine.ctx
        lpr, st_p = ctx.logprob_batch(q, _lib.MODE_LOGPRIOR)
        ll, st_l = ctx.logprob_batch(q, _lib.MODE_LOGLIKE)
        _raise_for_status(st_p, q)
        _raise_for_status(np.where(st_p != W_REJECT, st_l, 0), q)
        return lpr, ll

    def _draw_members(self, m):
        """The T members' general layouts of m iterations, stacked rung by rung: eight arrays (m, T, ...)."""
        per = [r._draw_steps(m) for r in self._rungs]
        return [np.stack([p[i] for p in per], axis=1) for i in range(8)]

    def _draw_swaps(self, m):
        return [draw_swap_logu(self._swap_rng, m, self.ntemps, self.nwalkers)]

    def sample(self, initial_state, iterations=1, store=True, adapt=None):
        from .engine import _raise_for_status
        coords, ll, lpr = self._start(initial_state)
        if int(iterations) <= 0:
            return
        ctx = self.engine.ctx
        adapt = self._adapting(adapt)
        base_acc, base_swap, base_skipped = self._accepted.copy(), self._nswap.copy(), self.ladder_skipped
        fixed = self.betas

        def enqueue(slot, m, arrays):
            if adapt:
                self._adapted += m
            if arrays is None:
                ctx.tempered_enqueue_drawn(slot, m, self.seeds, self._moves, self._drawn)
                self._drawn += m
            else:
                ctx.tempered_enqueue(slot, *arrays)

        ctx.sampler_policy(0)   # plain launches: the overlapped hand-over is part of the fused proposal
        ctx.tempered_begin(self.betas, coords, ll, lpr, self.chunk)
        if store and self._series is not None:
            try:
                ctx.tempered_attach_series(self._series, self._dens, len(self._chain))   # (rows a consumer never saw are overwritten)
            except Exception:
                ctx.tempered_end()
                raise
        collect, end = ctx.tempered_collect, ctx.tempered_end
        if adapt:   # (a fixed run calls none of the three)
            try:
                ctx.tempered_adapt(self.adaptation_lag, self.adaptation_time, self._adapted)
            except Exception:
                ctx.tempered_end()
                raise

            def collect(slot, m):
                return ctx.tempered_collect(slot, m) + (ctx.tempered_betas(slot, m),)

            def end():   # the device's ladder behind everything queued, whether the loop finished or was left
                try:
                    self.betas, _, skipped = ctx.tempered_ladder()
                    self.ladder_skipped = base_skipped + skipped
                finally:
                    ctx.tempered_end()
        draws = None if self.rng_mode == 'device' else (self._draw_members, self._draw_swaps)
        with closing(_pump(iterations, self.chunk, draws, enqueue, collect, end)) as chunks:
            for mm, (chain, llc, lprc, nacc, nswap, worst, *rows) in chunks:
                bad = np.nonzero(np.asarray(worst) > W_REJECT)[0]
                if bad.size:
                    _raise_for_status(np.array([worst[bad[0]]]), chain[-1][int(bad[0])][:1])
                self._accepted = base_acc + nacc
                self._nswap = base_swap + nswap
                for i in range(mm):
                    self.iteration += 1
                    if store:
                        self._betas_rows.append(rows[0][i].copy() if rows else fixed)
                        self._chain.append(chain[i])
                        self._ll.append(llc[i])
                        self._lpr.append(lprc[i])
                    self._last = TemperedState(chain[i], llc[i], lprc[i])
                    yield self._last


# ---- every target's ladder in one run ------------------------------------------------------------------
def _per_target(value, K, name):
    """``value`` once per target: a scalar for all, or a sequence of K."""
    if not isinstance(value, (list, tuple, np.ndarray)):
        return [value] * K
    if len(value) != K:
        raise ValueError('{}: one per target ({} given, {} targets)'.format(name, len(value), K))
    return list(value)


def _target_betas(K, ntemps, betas, beta_min):
    """K ladders of one length: ``betas`` is one ladder for all targets (1-D), one per target (K rows) or None (geometric)."""
    if betas is None or np.ndim(betas[0]) == 0:
        per = [resolve_betas(ntemps, betas, beta_min)] * K
    else:
        if len(betas) != K:
            raise ValueError('betas: one ladder for all targets or one per target')
        per = [resolve_betas(ntemps, b, beta_min) for b in betas]
    if len({len(b) for b in per}) != 1:
        raise ValueError('the targets of a group share ntemps')
    if K * len(per[0]) > MAX_TEMPS:
        raise ValueError('targets x rungs must not exceed {} ({} x {} asked for)'.format(MAX_TEMPS, K, len(per[0])))
    return per


def _seed_args(s):
    """``seeds[k]`` as a ladder's (seed, seeds): one key (rung t gets key + t) or one per rung."""
    return (s, None) if s is None or np.ndim(s) == 0 else (None, list(s))


def _named(k, fn, *a):
    """fn(*a) with a walker error prefixed ``target k:`` (as TargetGroup and DeviceGroupSampler name theirs)."""
    try:
        return fn(*a)
    except (KeyError, IndexError, ValueError, RuntimeError) as e:
        raise type(e)('target {}: {}'.format(k, e.args[0] if e.args else e)) from None


class GroupTemperedSampler:
    """K host ``TemperedSampler``s stepped in lock-step -- the definition of a group's tempered run.  Target k keeps its own
    ``nwalkers[k]``, ``betas[k]``, ``seeds[k]`` (one key, or one per rung), moves and adaptation parameters; per half-step the
    K x T rungs' proposals are evaluated in TWO batched calls, ``logprior_fn(list_of_K_arrays)`` and ``loglike_fn(...)``, each
    returning K arrays of values or K ``(values, statuses)``.  A ``TargetGroup`` in ``loglike_fn``'s place (``logprior_fn=None``)
    stands for its two status-carrying launches.  Everything else -- the status rule, the accept rule, the sweep, the ladder
    step -- is ``TemperedSampler``'s own code on target k's own state, so target k's chain is ``TemperedSampler``'s on target k
    alone.  ``draws``: one ``draws(first_iteration, m)`` per target (``TemperedSampler(draws=...)``).  ``target(k)``: target k's
    ``TemperedSampler``, with the whole ladder interface."""

    def __init__(self, nwalkers, ndim, loglike_fn, logprior_fn=None, ntemps=None, betas=None, beta_min=0.02, seeds=None, moves=None,
                 draws=None, adaptive=False, adaptation_lag=10000.0, adaptation_time=100.0):
        nwalkers = [int(n) for n in nwalkers]
        K = len(nwalkers)
        engines = [None] * K
        if logprior_fn is None and hasattr(loglike_fn, 'engines'):
            from . import _lib
            grp = loglike_fn
            engines = grp.engines
            loglike_fn, logprior_fn = (lambda qs: _group_eval(grp, qs, _lib.MODE_LOGLIKE)), (lambda qs: _group_eval(grp, qs, _lib.MODE_LOGPRIOR))
        if len(engines) != K:
            raise ValueError('one walker count per target ({} given, {} targets)'.format(K, len(engines)))
        self.loglike_fn, self.logprior_fn = loglike_fn, logprior_fn
        self.ndim = int(ndim)
        per_betas = _target_betas(K, ntemps, betas, beta_min)
        seeds, draws = _per_target(seeds, K, 'seeds') if seeds is not None else [None] * K, _per_target(draws, K, 'draws')
        lags, times = _per_target(adaptation_lag, K, 'adaptation_lag'), _per_target(adaptation_time, K, 'adaptation_time')
        self._now = [None] * K   # the batched evaluation's results, handed to target k's own status rule
        self.targets = []
        for k in range(K):
            seed, sds = _seed_args(seeds[k])
            s = TemperedSampler(nwalkers[k], ndim, (lambda q, k=k: self._now[k][1]), (lambda q, k=k: self._now[k][0]), betas=per_betas[k],
                                seed=seed, seeds=sds, moves=moves, draws=draws[k], adaptive=adaptive, adaptation_lag=lags[k],
                                adaptation_time=times[k])
            s.engine = engines[k]
            self.targets.append(s)
        self.ntemps = self.targets[0].ntemps

    @property
    def nwalkers(self):
        return [s.nwalkers for s in self.targets]

    def target(self, k):
        return self.targets[int(k)]

    def reset(self):
        for s in self.targets:
            s.reset()

    def _evaluate(self, qs):
        """(lpr, ll) per target of K arrays of proposals (an empty array: a target with nothing to evaluate): two batched
        calls, then each target's own status rule."""
        lprs, lls = self.logprior_fn(qs), self.loglike_fn(qs)
        if len(lprs) != len(qs) or len(lls) != len(qs):
            raise ValueError('a density function returned the wrong number of targets')
        out = []
        for k, s in enumerate(self.targets):
            if len(qs[k]) == 0:
                out.append(None)
                continue
            self._now[k] = (lprs[k], lls[k])
            out.append(_named(k, s._evaluate, qs[k]))
        return out

    def _start(self, initial_states):
        if len(initial_states) != len(self.targets):
            raise ValueError('one initial state per target')
        qs = []
        for s, st in zip(self.targets, initial_states):   # the targets that come as coordinates are evaluated in one batch
            flat = np.empty((0, self.ndim))
            if not isinstance(st, TemperedState):
                c = np.array(st, dtype=float)
                c = np.repeat(c[None], s.ntemps, axis=0) if c.ndim == 2 else c
                if c.shape == (s.ntemps, s.nwalkers, self.ndim) and np.all(np.isfinite(c)):
                    flat = c.reshape(-1, self.ndim)
            qs.append(flat)
        if any(len(q) for q in qs):
            lprs, lls = self.logprior_fn(qs), self.loglike_fn(qs)
            for k in range(len(qs)):
                self._now[k] = (lprs[k], lls[k])
        return [_named(k, s._start, st) for k, (s, st) in enumerate(zip(self.targets, initial_states))]

    def sample(self, initial_states, iterations=1, store=True, adapt=None):
        """``initial_states``: one per target, what ``TemperedSampler.sample`` takes.  Yields a list of K TemperedStates."""
        state = self._start(initial_states)
        for _ in range(int(iterations)):
            drawn = [s._draw_steps(1) for s in self.targets]
            accepted = [np.zeros((s.ntemps, s.nwalkers), dtype=bool) for s in self.targets]
            before = [s._nswap.copy() for s in self.targets]
            for h in (0, 1):
                qs = [np.concatenate([_propose(coords[t], members[t], h) for t in range(s.ntemps)])
                      for s, (coords, _, _), (members, _) in zip(self.targets, state, drawn)]
                for k, (s, (lpr_q, ll_q)) in enumerate(zip(self.targets, self._evaluate(qs))):
                    coords, ll, lpr = state[k]
                    members, ns = drawn[k][0], s.nwalkers // 2
                    for t in range(s.ntemps):
                        sl = slice(t * ns, (t + 1) * ns)
                        _accept_rung(s.betas[t], coords[t], ll[t], lpr[t], accepted[k][t], members[t], h, qs[k][sl], lpr_q[sl], ll_q[sl])
            out = []
            for k, s in enumerate(self.targets):
                coords, ll, lpr = state[k]
                betas = s.betas
                swap_sweep(betas[:-1] - betas[1:], coords, ll, lpr, np.asarray(drawn[k][1])[0], s._nswap)
                if s._adapting(adapt):
                    s.betas, skipped = ladder_step(betas, s._nswap - before[k], s.nwalkers, s._adapted, s.adaptation_lag, s.adaptation_time)
                    s._adapted += 1
                    s.ladder_skipped += skipped
                s._accepted += accepted[k]
                s.iteration += 1
                if store:
                    s._betas_rows.append(betas)
                    s._chain.append(coords.copy())
                    s._ll.append(ll.copy())
                    s._lpr.append(lpr.copy())
                s._last = TemperedState(coords, ll, lpr)
                out.append(s._last)
            yield out

    def run_mcmc(self, initial_states, nsteps, **kw):
        st = None
        for st in self.sample(initial_states, iterations=nsteps, **kw):
            pass
        return st


def _group_eval(group, qs, mode):
    """K ``(values, statuses)`` of one launch of a ``TargetGroup`` over K arrays of walkers, statuses not raised."""
    arrs, counts, theta = group._stack(qs)
    if theta.shape[0] == 0:
        return [(np.empty(0), np.empty(0, dtype=np.int32)) for _ in arrs]
    logp, status = group.group.logprob_batch(theta, counts, mode)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
    return [(logp[off[k]:off[k + 1]].copy(), status[off[k]:off[k + 1]].copy()) for k in range(len(arrs))]


class _TargetLadder(_Ladder):
    """``DeviceGroupTemperedSampler.target(k)``: target k's ladder -- its stored rows, counts, generators and the whole
    ``_Ladder`` interface.  With the run's series on the device (K T members) its T rungs are the view's own members (``_stored``)."""

    def __init__(self, parent, k, nwalkers, betas, seed, seeds, moves, adaptive, lag, time):
        self.parent, self.k = parent, int(k)
        self.engine = parent.group.engines[k]
        self._init_ladder(nwalkers, parent.ndim, None, betas, None, seed, seeds, moves, adaptive, lag, time)

    _series = property(lambda self: self.parent._series)
    _dens = property(lambda self: self.parent._dens)
    _device_modes = True
    _evaluate = DeviceTemperedSampler._evaluate

    def _stored(self):
        """_Ladder's view; with the run's series on the device its T rungs are the view's own among the K T members (each
        target's rungs with the target's engine).  With autocorr='host' its own T rungs alone are uploaded."""
        if self._series is None:
            return super()._stored()
        T, par = self.ntemps, self.parent
        return StoredChain(self._series, self._flat_members, len(self._chain), self.ndim, [n for n in par.nwalkers for _ in range(T)],
                           [e for e in par.group.engines for _ in range(T)], range(self.k * T, (self.k + 1) * T), device_modes=True, joined=True)


class DeviceGroupTemperedSampler:
    """Every target's ladder resident on the GPU in ONE run (``msx_group_tempered_*``; csrc/group_tempered_kernels.h; DESIGN.md
    section 20): K targets x T rungs are the members of one ensemble, and an iteration takes eight launches for ALL targets
    (nine when adaptive) where K ``DeviceTemperedSampler``s take eight each.  ``group`` is a ``TargetGroup``; ``nwalkers``
    walkers per rung, one count per target; ``betas`` one ladder for all targets or one per target (one ``ntemps`` for the group,
    K x ntemps <= 64); ``seeds[k]`` target k's key (rung t gets key + t) or its T keys; ``adaptation_lag`` / ``adaptation_time``
    one for all or one per target.  Target k's chain is bit for bit ``DeviceTemperedSampler``'s on ``group.engines[k]`` alone
    with ``seeds[k]`` -- whatever ``rng``, ``autocorr`` and ``adaptive`` are -- and so ``TemperedSampler``'s and
    ``GroupTemperedSampler``'s.

    ``target(k)`` is target k's ladder with ``_Ladder``'s interface (``get_chain(t)``, ``get_log_like``, ``get_betas``,
    ``acceptance_fraction``, ``swap_fraction``, ``get_autocorr_time``, ``get_summary``, ``get_products``, ``mean_log_like``,
    ``log_evidence``, ...).  ``autocorr='device'``: the rows are kept in ONE pair of device series of K T members and those
    calls work there.  ``_drawn`` and ``_adapted`` (each target's) follow ``DeviceTemperedSampler``'s rules: they count the
    iterations QUEUED, ``reset()`` leaves them alone, and after a run ends each target's ``betas`` is the device's ladder behind
    everything queued.  A walker error raises what ``DeviceTemperedSampler`` raises, prefixed ``target k:``."""

    def __init__(self, group, nwalkers, ndim, ntemps=None, betas=None, beta_min=0.02, seeds=None, chunk=64, rng='host', moves=None,
                 autocorr='host', cap_hint=0, adaptive=False, adaptation_lag=10000.0, adaptation_time=100.0):
        if rng not in ('host', 'device'):
            raise ValueError("rng must be 'host' or 'device'")
        if autocorr not in ('host', 'device'):
            raise ValueError("autocorr must be 'host' or 'device'")
        nwalkers = [int(n) for n in nwalkers]
        K = len(nwalkers)
        if K != len(group):
            raise ValueError('one walker count per target ({} given, {} targets)'.format(K, len(group)))
        if int(chunk) < 1:
            raise ValueError('chunk must be at least 1')
        self.group, self.ndim, self.chunk, self.rng_mode, self.autocorr = group, int(ndim), int(chunk), rng, autocorr
        self.adaptive = bool(adaptive)
        per_betas = _target_betas(K, ntemps, betas, beta_min)
        seeds = _per_target(seeds, K, 'seeds') if seeds is not None else [None] * K
        lags, times = _per_target(adaptation_lag, K, 'adaptation_lag'), _per_target(adaptation_time, K, 'adaptation_time')
        self._series = self._dens = None
        self.targets = []
        for k in range(K):
            seed, sds = _seed_args(seeds[k])
            self.targets.append(_TargetLadder(self, k, nwalkers[k], per_betas[k], seed, sds, moves, adaptive, lags[k], times[k]))
        self.ntemps = self.targets[0].ntemps
        self._moves = self.targets[0]._moves
        if autocorr == 'device':
            from . import _lib
            counts = [n for n in nwalkers for _ in range(self.ntemps)]
            ctx = group.engines[0].ctx
            self._series = _lib.Series(ctx, sum(counts), self.ndim, counts, cap_hint=int(cap_hint))
            self._dens = _lib.Series(ctx, sum(counts), 2, counts, cap_hint=int(cap_hint))

    @property
    def nwalkers(self):
        return [v.nwalkers for v in self.targets]

    def target(self, k):
        return self.targets[int(k)]

    def reset(self):
        """Forget every target's stored chain and counts; the streams' positions, ``_drawn`` and ``_adapted`` are left alone."""
        for v in self.targets:
            v.reset()

    def _draw_members(self, m):
        """The K T members' general layouts of m iterations, side by side in member order: kind (m, K T), the others (m, 2, H)."""
        per = [r._draw_steps(m) for v in self.targets for r in v._rungs]
        return [np.stack([p[i] for p in per], axis=1) if i == 2 else np.concatenate([p[i] for p in per], axis=2) for i in range(8)]

    def _draw_swaps(self, m):
        return [np.concatenate([draw_swap_logu(v._swap_rng, m, v.ntemps, v.nwalkers).reshape(int(m), -1) for v in self.targets], axis=1)]

    def sample(self, initial_states, iterations=1, store=True, adapt=None):
        """``initial_states``: one per target -- a TemperedState, or coordinates (nw_k, ndim) / (T, nw_k, ndim).  Yields a list
        of K TemperedStates per iteration."""
        from .engine import _raise_for_status
        if len(initial_states) != len(self.targets):
            raise ValueError('one initial state per target')
        start = [_named(k, v._start, st) for k, (v, st) in enumerate(zip(self.targets, initial_states))]
        if int(iterations) <= 0:
            return
        grp, T, ndim = self.group.group, self.ntemps, self.ndim
        adapt = self.adaptive if adapt is None else bool(adapt)
        counts = self.nwalkers
        off = np.concatenate([[0], np.cumsum([T * n for n in counts])]).astype(int)
        base = [(v._accepted.copy(), v._nswap.copy(), v.ladder_skipped, v.betas) for v in self.targets]

        def enqueue(slot, m, arrays):
            if adapt:
                for v in self.targets:
                    v._adapted += m
            if arrays is None:
                grp.tempered_enqueue_drawn(slot, m, [v.seeds for v in self.targets], self._moves, self.targets[0]._drawn)
                for v in self.targets:
                    v._drawn += m
            else:
                grp.tempered_enqueue(slot, *arrays)

        grp.tempered_begin(np.array([v.betas for v in self.targets]), counts, np.concatenate([c.reshape(-1, ndim) for c, _, _ in start]),
                           np.concatenate([ll.ravel() for _, ll, _ in start]), np.concatenate([lpr.ravel() for _, _, lpr in start]), self.chunk)
        collect, end = grp.tempered_collect, grp.tempered_end
        try:
            if store and self._series is not None:
                grp.tempered_attach_series(self._series, self._dens, len(self.targets[0]._chain))   # (rows a consumer never saw are overwritten)
            if adapt:   # (a fixed run calls none of the three)
                grp.tempered_adapt([v.adaptation_lag for v in self.targets], [v.adaptation_time for v in self.targets],
                                   [v._adapted for v in self.targets])

                def collect(slot, m):
                    return grp.tempered_collect(slot, m) + (grp.tempered_betas(slot, m),)

                def end():   # the device's ladders behind everything queued, whether the loop finished or was left
                    try:
                        betas, _, skipped = grp.tempered_ladder()
                        for k, v in enumerate(self.targets):
                            v.betas, v.ladder_skipped = betas[k].copy(), base[k][2] + int(skipped[k])
                    finally:
                        grp.tempered_end()
        except Exception:
            grp.tempered_end()
            raise
        draws = None if self.rng_mode == 'device' else (self._draw_members, self._draw_swaps)
        with closing(_pump(iterations, self.chunk, draws, enqueue, collect, end)) as chunks:
            for mm, (chain, llc, lprc, nacc, nswap, worst, *rows) in chunks:
                per = []
                for k, v in enumerate(self.targets):
                    sl, shp = slice(off[k], off[k + 1]), (mm, T, v.nwalkers)
                    per.append((chain[:, sl].reshape(shp + (ndim,)), llc[:, sl].reshape(shp), lprc[:, sl].reshape(shp)))
                    bad = np.nonzero(worst[k] > W_REJECT)[0]
                    if bad.size:
                        _named(k, _raise_for_status, np.array([worst[k][bad[0]]]), per[k][0][-1][int(bad[0])][:1])
                for k, v in enumerate(self.targets):
                    v._accepted = base[k][0] + nacc[off[k]:off[k + 1]].reshape(T, v.nwalkers)
                    v._nswap = base[k][1] + nswap[k]
                for i in range(mm):
                    out = []
                    for k, v in enumerate(self.targets):
                        c, ll, lpr = per[k]
                        v.iteration += 1
                        if store:
                            v._betas_rows.append(rows[0][i, k].copy() if rows else base[k][3])
                            v._chain.append(c[i])
                            v._ll.append(ll[i])
                            v._lpr.append(lpr[i])
                        v._last = TemperedState(c[i], ll[i], lpr[i])
                        out.append(v._last)
                    yield out

    def run_mcmc(self, initial_states, nsteps, **kw):
        st = None
        for st in self.sample(initial_states, iterations=nsteps, **kw):
            pass
        return st
