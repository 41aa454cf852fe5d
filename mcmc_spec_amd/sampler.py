"""A minimal ensemble sampler speaking the emcee protocol the reference drives.

The reference's sampler block (mft6.py:1490-1529, commented out in the snapshot) needs:
``EnsembleSampler(nwalkers, ndim, log_prob_fn, args=, kwargs=)``, ``sample(pos, iterations=)`` yielding
states with ``.coords``, ``get_last_sample()``, ``reset()``, ``get_autocorr_time(quiet=True)``,
``acceptance_fraction`` and ``chain``.  emcee is not installed here, so this module restates the
published algorithm -- Goodman & Weare (2010) affine-invariant stretch move as emcee 3 applies it by
default: the ensemble is split into two random halves that are updated in turn, each walker proposing
``q = c - z (c - s)`` against a random walker ``c`` of the other half with
``z = ((a-1) u + 1)^2 / a`` and acceptance ``(ndim-1) ln z + ln p(q) - ln p(s)``.

With ``vectorize=True`` the log-probability function receives the whole half-ensemble as an
``(n, ndim)`` array -- one fused GPU launch per half-step with ``mcmc_spec_amd.mft6.logposterior``.
"""
from __future__ import annotations

import warnings
from collections import deque
from contextlib import closing
from concurrent.futures import ThreadPoolExecutor

import numpy as np


class State:
    def __init__(self, coords, log_prob, random_state=None):
        self.coords = np.array(coords, dtype=float)
        self.log_prob = np.array(log_prob, dtype=float)
        self.random_state = random_state

    def __iter__(self):  # emcee allows `pos, lnp, rstate = state`
        return iter((self.coords, self.log_prob, self.random_state))


def counter_draws(seed, a, ndim, first_iter, m, nwalkers):
    """NumPy restatement of the DEVICE generator (csrc/logprob_kernel.h, sampler_draw_kernel): the randomness of
    iterations ``first_iter .. first_iter + m - 1`` of a run keyed by ``seed`` -- every number a pure function of (seed,
    iteration, stream, index) through SplitMix64's output function.  Returns what ``EnsembleSampler._draw_steps`` returns:
    ``sidx, cidx, partner`` (int32) and ``zz, zfac, logu`` (float64), each (m, 2, nwalkers / 2).  Indices and ``zz`` equal
    the device's bit for bit; ``zfac`` / ``logu`` go through NumPy's ``log`` instead of the device's (last-place
    differences), which is why the device-drawn chain is checked against the host loop fed with ``msx_sampler_draw``'s
    arrays, and this restatement against those arrays (tests/test_gpu_overlap.py)."""
    nw, ns = int(nwalkers), int(nwalkers) // 2
    sidx, cidx, uniform = counter_streams(seed, first_iter, m, nw)
    uz, up, ua = (np.stack([uniform(k + 3 * h, ns) for h in (0, 1)], axis=1) for k in (1, 2, 3))
    t1 = (float(a) - 1.0) * uz + 1.0
    zz = (t1 * t1) / float(a)
    partner = np.minimum((up * ns).astype(np.int32), ns - 1)
    with np.errstate(divide='ignore'):
        logu = np.log(ua)
    zfac = (float(ndim) - 1.0) * np.log(zz)
    return sidx, cidx, partner, zz, zfac, logu


def counter_streams(seed, first_iter, m, nwalkers):
    """The counter generator's pieces for iterations ``first_iter .. first_iter + m - 1`` of ``seed``: ``sidx, cidx`` (the
    split: the walkers sorted by stream 0's keys) and ``uniform(stream, n)`` -> (m, n), the uniforms of indices 0..n-1 of
    one stream.  Shared by ``counter_draws`` and ``moves.counter_draws_moves``."""
    nw, ns = int(nwalkers), int(nwalkers) // 2
    u64 = np.uint64
    seed = u64(int(seed) & 0xffffffffffffffff)

    def mix(it, stream, index):
        with np.errstate(over='ignore'):
            ctr = (it.astype(u64) << u64(28)) + (u64(stream) << u64(24)) + index.astype(u64)
            x = seed * u64(0xD1342543DE82EF95) + (ctr + u64(1)) * u64(0x9E3779B97F4A7C15)
            x ^= x >> u64(30); x *= u64(0xBF58476D1CE4E5B9)
            x ^= x >> u64(27); x *= u64(0x94D049BB133111EB)
            x ^= x >> u64(31)
        return x

    it = (np.arange(m, dtype=np.int64) + int(first_iter))[:, None]

    def uniform(stream, n):
        k = mix(np.broadcast_to(it, (m, n)), stream, np.broadcast_to(np.arange(n)[None, :], (m, n)))
        return (k >> u64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)

    keys = mix(np.broadcast_to(it, (m, nw)), 0, np.broadcast_to(np.arange(nw)[None, :], (m, nw)))
    perm = np.argsort(keys, axis=1, kind='stable').astype(np.int32)      # sorted by (key, index)
    halves = perm.reshape(m, 2, ns)
    return np.ascontiguousarray(halves), np.ascontiguousarray(halves[:, ::-1]), uniform


def device_seed(seed):
    """The device generator's 64-bit key for a sampler's ``seed`` (``DeviceEnsembleSampler.device_seed``, one per target in
    ``DeviceGroupSampler.device_seeds``): an int as itself, masked to 64 bits; None (fresh entropy), a ``SeedSequence`` or a
    sequence of ints -- whatever ``EnsembleSampler`` takes for its own generators -- through
    ``SeedSequence.generate_state(1, uint64)``."""
    if isinstance(seed, (int, np.integer)):
        return int(seed) & 0xffffffffffffffff
    ss = seed if isinstance(seed, np.random.SeedSequence) else np.random.SeedSequence(seed)
    return int(ss.generate_state(1, dtype=np.uint64)[0]) & 0xffffffffffffffff


class EnsembleSampler:
    def __init__(self, nwalkers, ndim, log_prob_fn, args=None, kwargs=None, a=None, vectorize=False, pool=None,
                 threads=None, seed=None, draws=None, moves=None, _general=False):
        """``moves`` (optional): a ``moves.StretchMove`` / ``moves.DEMove``, a list of them (equal weights) or a list of
        ``(move, weight)`` -- emcee's ``moves=``; each iteration takes one move of the set, chosen with the normalised
        weights.  None, or a ``StretchMove`` alone, is the stretch move through the code path it has always had (``a=`` and
        ``moves=`` exclude each other); a set with another move goes through the general propose / accept
        (``mcmc_spec_amd.moves``).

        ``draws(first_iteration, m)`` (optional) replaces the sampler's own generators: it returns the randomness of
        ``m`` iterations in ``_draw_steps``' layout -- e.g. ``lambda i, m: ctx.sampler_draw(seed, a, i, m, nwalkers, ndim)``
        makes this host loop walk the chain the device-resident sampler draws for itself (``rng='device'``)."""
        self._draws = draws
        self._drawn = 0
        a, self._moves = _resolve_moves(a, moves, _general)
        if nwalkers < 2 * ndim or nwalkers % 2:
            raise ValueError('the stretch move needs an even number of walkers >= 2*ndim')
        if self._moves is not None and not self._moves.pure_stretch and nwalkers < 4:
            raise ValueError('the DE move needs two distinct walkers in each half: at least 4 walkers')
        if threads is not None:
            warnings.warn('threads= is an emcee-2 argument and is ignored (as in emcee 3)', DeprecationWarning)
        self.nwalkers, self.ndim = int(nwalkers), int(ndim)
        self.log_prob_fn = log_prob_fn
        self.args = list(args or [])
        self.kwargs = dict(kwargs or {})
        self.a = a
        self.vectorize = bool(vectorize)
        self.pool = pool
        # two independent streams of one seed: uniforms (stretch factors, partners, accept draws) and the
        # random split.  Each is consumed strictly row by row, so drawing m iterations in one call gives the
        # same numbers as m calls of one iteration -- the host loop (m = 1) and the device-resident loop
        # (m = chunk) walk the same chain
        ss = seed if isinstance(seed, np.random.SeedSequence) else np.random.SeedSequence(seed)
        self.rng, self._rng_split = (np.random.Generator(np.random.PCG64(c)) for c in ss.spawn(2))
        self.reset()

    # ---- bookkeeping ------------------------------------------------------------------------------
    def reset(self):
        self._chain = []
        self._logp = []
        self._accepted = np.zeros(self.nwalkers)
        self.iteration = 0
        self._last = None

    @property
    def chain(self):
        """(nwalkers, nsteps, ndim), the layout ``sampler.chain`` has in the reference (mft6.py:1527)."""
        if not self._chain:
            return np.empty((self.nwalkers, 0, self.ndim))
        return np.swapaxes(np.array(self._chain), 0, 1)

    def get_chain(self, flat=False, thin=1, discard=0):
        c = np.array(self._chain)[discard::thin]
        return c.reshape(-1, self.ndim) if flat else c

    def get_log_prob(self, flat=False, thin=1, discard=0):
        lp = np.array(self._logp)[discard::thin]
        return lp.reshape(-1) if flat else lp

    @property
    def acceptance_fraction(self):
        return self._accepted / max(self.iteration, 1)

    def get_last_sample(self):
        return self._last

    # ---- probability calls --------------------------------------------------------------------------
    def compute_log_prob(self, coords):
        coords = np.asarray(coords, dtype=float)
        if np.any(~np.isfinite(coords)):
            raise ValueError('At least one parameter value was infinite or NaN')
        if self.vectorize:
            lp = np.asarray(self.log_prob_fn(coords, *self.args, **self.kwargs), dtype=float)
        else:
            mapper = self.pool.map if self.pool is not None else map
            lp = np.array([float(v) for v in mapper(_Call(self.log_prob_fn, self.args, self.kwargs), coords)])
        if lp.shape != (len(coords),):
            raise ValueError('log_prob_fn returned the wrong shape')
        if np.any(np.isnan(lp)):
            raise ValueError('Probability function returned NaN')
        return lp

    # ---- the move -------------------------------------------------------------------------------------
    def _draw_steps(self, m):
        """All randomness of ``m`` iterations at once: per iteration the random split into two halves, then per
        half the stretch factors ``z = ((a-1)u+1)^2/a``, the partner index ``floor(u*n_half)`` and ``ln u`` of
        the accept draw.  Returns ``sidx, cidx, partner`` (int32) and ``zz, zfac, logu`` (float64), each of
        shape (m, 2, nwalkers/2); ``zfac = (ndim-1) ln z``.  Shared by the host loop and the device-resident
        loop; everything is vectorised over the m iterations (the host must stay ahead of a 23 us kernel).
        A sampler with a set of moves returns the general layout instead: ``sidx, cidx, kind[m], p1, p2, g, fac, logu``
        (``mcmc_spec_amd.moves``)."""
        if self._draws is not None:
            out = self._draws(self._drawn, m)
            self._drawn += m
            return out
        return self._draw_split(m) + self._draw_moves(m)

    def _draw_split(self, m):
        """(sidx, cidx): the random split of each of m iterations (stream ``_rng_split``)."""
        nw, ns = self.nwalkers, self.nwalkers // 2
        # permuted() has its fast path for 8-byte items
        perm = self._rng_split.permuted(np.broadcast_to(np.arange(nw, dtype=np.int64), (m, nw)).copy(), axis=1)
        halves = perm.astype(np.int32).reshape(m, 2, ns)
        return halves, halves[:, ::-1]

    def _draw_moves(self, m):
        """(partner, zz, zfac, logu) of m iterations (stream ``rng``); with a set of moves the general layout's (kind, p1,
        p2, g, fac, logu) -- ``moves.general_draws``.  Per iteration the generator yields the stretch move's 3 x 2 x ns
        uniforms and, for a set with a DE move, one more for the move's choice and 3 x 2 x ns for the pairs and the
        normal deviates: row by row, so m iterations at once are m calls of one, and a pure-stretch set consumes the
        stream exactly as the default move does."""
        ns = self.nwalkers // 2
        if self._moves is not None:
            from . import moves as mv
            mset, n6 = self._moves, 6 * ns
            u = self.rng.random((m, n6 if mset.pure_stretch else 2 * n6 + 1))
            uz, up, ua = (np.ascontiguousarray(u[:, :n6].reshape(m, 3, 2, ns)[:, j]) for j in range(3))
            if mset.pure_stretch:
                which, ud, u1, u2 = np.zeros(m, dtype=np.int32), None, None, None
            else:
                which = mv.choose_kind(mset, u[:, n6])
                ud, u1, u2 = (np.ascontiguousarray(u[:, n6 + 1:].reshape(m, 3, 2, ns)[:, j]) for j in range(3))
            return mv.general_draws(mset, self.ndim, ns, which, uz, up, ua, ud, u1, u2)
        u = self.rng.random((m, 3, 2, ns))
        # contiguous operands: the elementwise loops (log in particular) then take the same code path for
        # every m, which the bit-identity of host and device chains relies on
        uz, up, ua = (np.ascontiguousarray(u[:, j]) for j in range(3))
        zz = ((self.a - 1.0) * uz + 1.0) ** 2 / self.a
        partner = np.minimum((up * ns).astype(np.int32), ns - 1)
        with np.errstate(divide='ignore'):
            logu = np.log(ua)
        zfac = (self.ndim - 1.0) * np.log(zz)
        return partner, zz, zfac, logu

    def _stretch_step(self, coords, logp):
        accepted = np.zeros(self.nwalkers, dtype=bool)
        draws = self._draw_steps(1)
        for h in (0, 1):
            q = _propose(coords, draws, h)
            _accept(coords, logp, accepted, draws, h, q, self.compute_log_prob(q))
        return accepted

    def sample(self, initial_state, iterations=1, store=True):
        if isinstance(initial_state, State):
            coords, logp = initial_state.coords.copy(), initial_state.log_prob.copy()
        else:
            coords, logp = np.array(initial_state, dtype=float), None
        if coords.shape != (self.nwalkers, self.ndim):
            raise ValueError('incompatible input dimensions')
        if logp is None or logp.shape != (self.nwalkers,):
            logp = self.compute_log_prob(coords)
        for _ in range(int(iterations)):
            acc = self._stretch_step(coords, logp)
            self._accepted += acc
            self.iteration += 1
            if store:
                self._chain.append(coords.copy())
                self._logp.append(logp.copy())
            self._last = State(coords, logp)
            yield self._last

    def run_mcmc(self, initial_state, nsteps, **kw):
        st = None
        for st in self.sample(initial_state, iterations=nsteps, **kw):
            pass
        return st

    # ---- diagnostics: every analysis is the stored-chain view's (mcmc_spec_amd.stored) ---------------
    def _stored(self):
        """The view of the stored chain that the analyses below ask."""
        from .stored import StoredChain
        return StoredChain(None, lambda members=None: np.array(self._chain), len(self._chain), self.ndim)

    def get_autocorr_time(self, quiet=False, c=5.0, tol=50.0, discard=0, thin=1):
        """Integrated autocorrelation time per dimension (Sokal window, like emcee's ``integrated_time``)."""
        return self._stored().autocorr_time(0, quiet, c, tol, discard, thin)

    def get_rhat(self, discard=0, thin=1, cols=None):
        """Split R-hat per column over the walkers of the stored chain, rows ``[discard::thin]`` (at least 4):
        ``diagnostics.split_rhat``.  ``cols``: coordinates; None for all.  DeviceEnsembleSampler with
        autocorr='device': from the chain on the device (msx_series_moments), without a download; rows the device holds past
        len(self._chain) -- queued chunks not consumed yet -- are not part of it."""
        return self._stored().moments(0, discard, thin, cols, False)['rhat']

    def get_moments(self, discard=0, thin=1, cols=None):
        """{'mean' (ncols,), 'cov' (ncols, ncols), 'count'}: the mean and covariance of
        ``get_chain(discard=, thin=, flat=True)`` (``diagnostics.moments``); DeviceEnsembleSampler with autocorr='device': from
        the chain on the device (get_rhat's rules)."""
        out = self._stored().moments(0, discard, thin, cols, rhat=False)
        return {name: out[name] for name in ('mean', 'cov', 'count')}

    def get_rank_rhat(self, discard=0, thin=1, cols=None):
        """{'bulk', 'folded', 'rhat'}, each (ncols,): the rank-normalised split R-hat of Vehtari et al. (2021) over the walkers
        of the stored chain, rows ``[discard::thin]`` (at least 4), its folded companion, which sees a walker of another scale,
        and their maximum (``diagnostics.rank_rhat``)."""
        return self._stored().rank_rhat(0, discard, thin, cols)

    def get_ess(self, discard=0, thin=1, cols=None, kind='bulk'):
        """The effective sample size (ncols,) of the stored chain's walkers taken together: ``kind`` 'bulk' (what the central
        quantiles are worth), 'tail' (the 5 % and 95 % quantiles) or 'mean' (``diagnostics.ess``)."""
        return self._stored().ess(0, discard, thin, cols, kind)

    def get_mcse(self, discard=0, thin=1, cols=None, q=(0.16, 0.5, 0.84)):
        """{'mean' (ncols,), 'quantiles' (ncols, len(q))}: the Monte-Carlo standard errors of the chain's mean and of its
        quantiles ``q`` -- how many digits of a published percentile are real (``diagnostics.mcse``)."""
        return self._stored().mcse(0, discard, thin, cols, q)

    def get_modes(self, ncomp=2, discard=0, thin=1, cols=None, **fit_kw):
        """The posterior's modes: a joint Gaussian mixture of ``ncomp`` components over the columns ``cols`` (None: all)
        of ``get_chain(discard=, thin=, flat=True)``, as a ``modes.ModeFit`` (one member) whose ``labels()``, ``split()``
        and ``summary()`` give every sample's mode and the per-mode quantiles (``mcmc_spec_amd.modes``; DESIGN.md section
        23).  ``fit_kw``: ``modes.fit``'s max_iter, tol, ridge, center, scale, split_col, split_at.  DeviceEnsembleSampler fits
        on the device (msx_series_modes, msx_series_mode_labels): with autocorr='device' on the chain held there, without a
        download (rows past len(self._chain) are not part of it); otherwise the host chain is uploaded first and the result
        keeps that copy until its ``close()``."""
        return self._stored().modes(None, ncomp, discard, thin, cols, **fit_kw)


def _min_ess(sampler):
    """min over the columns of a check's bulk and tail ESS, from one computation of both; NaN while the chain is shorter
    than 4 rows."""
    try:
        st = sampler._stored().rank_stats(0, ('bulk', 'tail'))
        return float(min(np.min(st['ess_bulk']), np.min(st['ess_tail'])))   # (np.min keeps a NaN)
    except ValueError:
        return float('nan')


def _window(f, c):
    """The Sokal window over the lags f[:L] of one dimension: (the first index idx with idx >= c * taus[idx], or None if
    no index of the prefix qualifies; taus = 2 cumsum(f) - 1).  cumsum is sequential, so the taus of a prefix are those
    of the full length: an index found in a prefix is the index the full length gives."""
    taus = 2.0 * np.cumsum(f) - 1.0
    m = np.arange(len(taus)) < c * taus
    return (int(np.argmin(m)) if np.any(~m) else None), taus


def _integrated_time(f, c):
    """tau per dimension from the whole normalised autocorrelation f (ndim, L): taus at the Sokal window, or at the last
    lag when no window is found (what get_autocorr_time has always done)."""
    tau = np.empty(len(f))
    for d in range(len(f)):
        win, taus = _window(f[d], c)
        tau[d] = taus[len(taus) - 1 if win is None else win]
    return tau


def _check_tau(tau, n, thin, tol, quiet):
    """get_autocorr_time's tol rule: a chain shorter than tol taus raises unless quiet.  (n: rows after discard / thin.)"""
    if np.any(tol * tau > n * thin):
        msg = 'The chain is shorter than {} times the integrated autocorrelation time'.format(tol)
        if not quiet:
            raise RuntimeError(msg)
    return tau


ACF_TILE = 320  # the first lag tile of a device window search (autocorr_kernels.h: one workgroup's lags); then doubling


def _device_integrated_time(series, n_total, c, discard, thin):
    """tau (k, ndim) of the chain a ``_lib.Series`` holds in its first n_total rows, thinned x = rows[discard::thin]
    (n' >= 4 rows), before ``*= thin``: lag tiles of growing length (ACF_TILE, 2 ACF_TILE, ... up to n') are requested
    for the dimensions whose window some member has not found yet, one msx_series_acf call per tile over all members.  A
    window found in the prefix is the one the full length gives (_window); none by n' -> the last lag, as on the host."""
    n = len(range(discard, n_total, thin))
    k, ndim = series.k, series.ndim
    tau = np.full((k, ndim), np.nan)
    pending = {(m, d) for m in range(k) for d in range(ndim)}
    prefix = np.empty((k, ndim, 0))
    lag0, tile = 0, ACF_TILE
    while pending:
        nlag = min(tile, n - lag0)
        f = series.acf(n_total, discard, thin, lag0, nlag, sorted({d for _, d in pending}))
        prefix = np.concatenate([prefix, f], axis=2)
        lag0 += nlag
        tile *= 2
        for m, d in sorted(pending):
            win, taus = _window(prefix[m, d], c)
            if win is None and lag0 < n:
                continue
            tau[m, d] = taus[n - 1 if win is None else win]
            pending.discard((m, d))
    return tau


# One half-step of a move, in two parts around the evaluation of the proposals (EnsembleSampler, and GroupSampler for
# each of its targets).  draws: _draw_steps' arrays for one iteration -- the stretch move's six (sidx, cidx, partner, zz,
# zfac, logu) or the general layout's eight (sidx, cidx, kind, p1, p2, g, fac, logu: mcmc_spec_amd.moves); h: the half.
def _propose(coords, draws, h):
    """The proposals q of half h: each active walker s stretched towards its partner in the other half, or (a DE
    iteration of the general layout) displaced by g times the difference of two walkers of the other half."""
    if len(draws) == 6:
        sidx, cidx, p1, g = (d[0, h] for d in draws[:4])
        de = False
    else:
        sidx, cidx, p1, p2, g = (draws[i][0, h] for i in (0, 1, 3, 4, 5))
        de = int(draws[2][0]) != 0
    s, c = coords[sidx], coords[cidx]
    if de:
        diff = c[p1] - c[p2]
        prod = g[:, None] * diff
        return s + prod
    partner = c[p1]
    return partner - (partner - s) * g[:, None]


def _accept(coords, logp, accepted, draws, h, q, new_lp):
    """The accept rule of half h, in place: walkers whose ln u < factor + ln p(q) - ln p(s) move to q (factor: the stretch
    move's (ndim-1) ln z, 0 for a DE iteration)."""
    s_idx, zfac, logu = draws[0][0, h], draws[-2][0, h], draws[-1][0, h]
    with np.errstate(invalid='ignore'):  # -inf - -inf = nan -> compares False -> rejected
        lnpdiff = zfac + new_lp - logp[s_idx]
    acc = logu < lnpdiff
    coords[s_idx[acc]] = q[acc]
    logp[s_idx[acc]] = new_lp[acc]
    accepted[s_idx[acc]] = True


def _resolve_moves(a, moves, general=False):
    """(a, MoveSet or None) of a sampler's ``a=`` and ``moves=``: None for the stretch move through its own path -- no
    ``moves=``, or a ``StretchMove`` alone (whose ``a`` is then the sampler's) unless ``general`` forces it through the
    general one (the tests' comparison of the two paths)."""
    if moves is None:
        return (2.0 if a is None else float(a)), None
    if a is not None:
        raise ValueError('a= and moves= exclude each other: give the stretch scale as moves.StretchMove(a)')
    from .moves import parse_moves
    mset = parse_moves(moves)
    a0 = next((m.a for m in mset.moves if m.kind == 0), 2.0)
    if len(mset) == 1 and mset.pure_stretch and not general:
        return a0, None
    return a0, mset


def _pump(iterations, chunk, draws, enqueue, collect, end):
    """The device-resident samplers' chunk pipeline: yields ``(m, collect(slot, m))`` per chunk of m iterations, in order.

    ``draws = (split, moves)``: callables of m that draw a chunk's randomness on the host (two threads; NumPy's
    generators and the ctypes calls release the GIL), or None for chunks the device draws itself.  The randomness of
    chunk i+1 is drawn and QUEUED on the GPU (``enqueue(slot, m, arrays)``, arrays None for device draws) while chunk i
    runs; chunk i is collected only after chunk i+1 has been queued, so the GPU never waits for the host between chunks.
    Host-drawn chunk sizes ramp up from 8 so the first launch does not wait for a whole chunk of randomness.  The run
    begun by the caller ends (``end()``) when the generator finishes, raises or is closed."""
    def submit(pool, m):
        return (pool.submit(draws[0], m), pool.submit(draws[1], m)) if draws is not None and m > 0 else None

    def next_size(prev, left):
        if draws is None:   # (nothing to wait for on the host: whole chunks from the start)
            return min(left, chunk)
        return min(left, chunk, max(8, 2 * prev))

    left = int(iterations)
    try:
        with ThreadPoolExecutor(max_workers=2) as pool:
            queued = deque()
            m = next_size(4, left)
            fut = submit(pool, m)
            slot = 0
            while left > 0 or queued:
                if left > 0:
                    arrays = None if fut is None else [x for f in fut for x in f.result()]
                    left -= m
                    m_next = next_size(m, left) if left > 0 else 0
                    fut = submit(pool, m_next)
                    enqueue(slot, m, arrays)
                    queued.append((slot, m))
                    slot ^= 1
                    m = m_next
                    if len(queued) < 2 and left > 0:
                        continue  # keep two chunks in flight
                sl, mm = queued.popleft()
                yield mm, collect(sl, mm)
    finally:
        end()


class DeviceEnsembleSampler(EnsembleSampler):
    """The same sampler with the walker state resident in HBM: ``chunk`` iterations are queued on the GPU
    back to back (per half-step: proposal kernel, fused log-probability launch, accept kernel;
    ``msx_sampler_run``) and only the chain comes back.  Randomness is drawn on the host with exactly the
    calls of ``EnsembleSampler``, so for the same seed both samplers produce the same chain, bit for bit.

    ``engine`` is a staged ``mcmc_spec_amd.engine.Engine``; ``mode`` selects ``'logposterior'`` or
    ``'loglikelihood'`` as the target density.

    With ``rng='device'`` the library draws every chunk on the GPU from ``device_seed`` and the ABSOLUTE iteration number
    ``_drawn``, which every chunk queued advances and ``reset()`` leaves alone -- as ``EnsembleSampler(draws=...)`` counts
    on the host.  Consecutive ``sample()`` / ``run_mcmc()`` calls therefore continue ONE stream (burn-in, ``reset()``,
    production: ``run_reference_protocol``), and the chain is the one
    ``EnsembleSampler(draws=lambda i, m: ctx.sampler_draw(device_seed, a, i, m, nwalkers, ndim))`` walks over the same
    calls (tests/test_gpu_sampler_runs.py).  The position counts iterations QUEUED, not consumed: a ``sample()`` loop
    left early (a ``break``, as ``run_reference_protocol`` does on convergence, or a walker error) leaves ``_drawn`` past
    the last iteration yielded -- by the chunks already queued -- while the host twin stops at the last iteration it
    stepped.  Both remain valid chains; a later run on the same sampler then matches a twin whose ``_drawn`` is set to
    this sampler's."""

    def __init__(self, nwalkers, ndim, engine, mode='logposterior', a=None, seed=None, chunk=64, shard=None, rng='host', overlap=None,
                 autocorr='host', moves=None, _general=False):
        """``shard = (rank, world)`` runs the SHARDED form: every rank holds the whole ensemble on
        its GPU, evaluates block ``rank`` of each half-step's proposals, one RCCL all-gather of the new
        log-probabilities crosses xGMI and every rank applies the accept rule for all walkers on the device.
        Every rank must construct the sampler with the SAME seed and start from the same state; every rank then
        holds the same chain, bit-identical to the unsharded one.  ``world > 1`` needs the engine's RCCL
        communicator (``mcmc_spec_amd.dist.init_engine_comm``)."""
        from . import _lib
        # rng = 'host' (default): the randomness is drawn by this object's NumPy generators, exactly the calls of
        # EnsembleSampler -- same seed, same chain as the host loop.  rng = 'device': the library draws it on the GPU with a
        # counter-based generator keyed by `seed` (msx_sampler_enqueue_drawn: one launch per chunk, nothing uploaded, every
        # rank of a sharded run draws the same numbers -- so a sharded run over world > 1 needs an explicit seed); the chain
        # is then the one the host loop walks when it is fed `ctx.sampler_draw(device_seed, a, first_iteration, m, nwalkers,
        # ndim)` (EnsembleSampler(draws=...)), across runs and reset() (the class docstring).  Up to 4096 walkers.
        # overlap = None: consecutive half-steps run concurrently when the library's rule allows (an unsharded run whose two
        # half-steps fit the chip together: include/msx.h, msx_sampler_policy); False: plain launches -- the choice for a
        # GPU shared with other work, where a waiting workgroup's producer may not get a CU (the chunk then fails with
        # MSX_W_HANDOVER after a bounded wait, a RuntimeError here, and the run has to be started again).
        # moves: EnsembleSampler's.  A set with a move other than the stretch move runs beside the fused kernel: a small kernel
        # proposes, the plain evaluation scores, a small kernel accepts (msx_sampler_enqueue_moves*) --
        # plain launches (overlapped is False: the overlapped hand-over is part of the fused proposal), one GPU.
        # autocorr = 'host' (default): get_autocorr_time is EnsembleSampler's (the chain on the host, one FFT per walker and
        # dimension).  'device': the sampler keeps its stored chain on the device as well (a _lib.Series that every
        # sample(store=True) run appends to, from row len(self._chain) on) and get_autocorr_time computes the
        # autocorrelation there (msx_series_acf).  Same tau up to roundoff, same window.
        if autocorr not in ('host', 'device'):
            raise ValueError("autocorr must be 'host' or 'device'")
        self.autocorr = autocorr
        self._series = None
        self.overlap_policy = -1 if overlap is None or overlap else 0
        if rng not in ('host', 'device'):
            raise ValueError("rng must be 'host' or 'device'")
        self.rng_mode = rng
        self.shard = None if shard is None else (int(shard[0]), int(shard[1]))
        if rng == 'device' and seed is None and self.shard is not None and self.shard[1] > 1:
            # (every rank would draw its own entropy and propose its own moves while gathering the others' log-probabilities)
            raise ValueError("rng='device' with shard=(rank, world > 1) needs a seed: every rank must draw the same stream")
        self.device_seed = device_seed(seed) if rng == 'device' else None   # (the generator's key; None: the host draws)
        self.overlapped = None   # set by the first chunk of a run: did its half-steps overlap (include/msx.h)?
        self.engine = engine
        self.mode = mode
        self._mode = {'logposterior': _lib.MODE_LOGPOST, 'loglikelihood': _lib.MODE_LOGLIKE}[mode]
        fn = engine.logposterior if mode == 'logposterior' else engine.loglikelihood
        super().__init__(nwalkers, ndim, fn, a=a, vectorize=True, seed=seed, moves=moves, _general=_general)
        if self._moves is not None:
            if self.shard is not None and self.shard[1] > 1:
                raise ValueError('moves=: the sharded run (shard=(rank, world > 1)) is stretch only')
            self.overlap_policy = 0
        self.chunk = int(chunk)
        if autocorr == 'device':
            self._series = _lib.Series(engine.ctx, self.nwalkers, self.ndim)

    def sample(self, initial_state, iterations=1, store=True):
        from .engine import _raise_for_status
        if isinstance(initial_state, State):
            coords, logp = initial_state.coords.copy(), initial_state.log_prob.copy()
        else:
            coords, logp = np.array(initial_state, dtype=float), None
        if coords.shape != (self.nwalkers, self.ndim):
            raise ValueError('incompatible input dimensions')
        if logp is None or logp.shape != (self.nwalkers,):
            logp = self.compute_log_prob(coords)
        coords = np.ascontiguousarray(coords)
        logp = np.ascontiguousarray(logp)
        ctx = self.engine.ctx
        if int(iterations) <= 0:
            return
        base_acc = self._accepted.copy()

        def enqueue(slot, m, arrays):
            if arrays is None:
                # the device draws: the stream at its absolute iteration, which only a queued chunk advances
                if self._moves is not None:
                    ctx.sampler_enqueue_moves_drawn(slot, m, self.device_seed, self._moves, self._drawn)
                else:
                    ctx.sampler_enqueue_drawn(slot, m, self.device_seed, self.a, self._drawn)
                self._drawn += m
            elif self._moves is not None:
                ctx.sampler_enqueue_moves(slot, *arrays)
            else:
                ctx.sampler_enqueue(slot, *arrays)
            self.overlapped = ctx.sampler_overlapped() == 1   # (half-steps on two streams: include/msx.h)

        ctx.sampler_policy(self.overlap_policy)
        ctx.sampler_begin(self._mode, coords, logp, self.chunk)
        if self.shard is not None and self._moves is None:   # (a set of moves runs on one GPU: world is 1, nothing to shard)
            ctx.sampler_shard(*self.shard)
        if store and self._series is not None:
            try:
                ctx.sampler_attach_series(self._series, len(self._chain))   # (rows a consumer never saw are overwritten)
            except Exception:
                ctx.sampler_end()
                raise
        draws = None if self.rng_mode == 'device' else (self._draw_split, self._draw_moves)
        with closing(_pump(iterations, self.chunk, draws, enqueue, ctx.sampler_collect, ctx.sampler_end)) as chunks:
            for mm, (chain, lpc, nacc, worst) in chunks:
                if worst:
                    _raise_for_status(np.array([worst]), chain[-1][:1])
                self._accepted = base_acc + nacc
                for i in range(mm):
                    self.iteration += 1
                    if store:
                        self._chain.append(chain[i])
                        self._logp.append(lpc[i])
                    self._last = State(chain[i], lpc[i])
                    yield self._last

    @property
    def acceptance_fraction(self):
        return self._accepted / max(self.iteration, 1)

    def _stored(self):
        """EnsembleSampler's view with the resident series (autocorr='device'), the engine, and the mode fit on the device."""
        from .stored import StoredChain
        return StoredChain(self._series, lambda members=None: np.array(self._chain), len(self._chain), self.ndim, engines=[self.engine],
                           device_modes=True)

    def get_autocorr_time(self, quiet=False, c=5.0, tol=50.0, discard=0, thin=1):
        """EnsembleSampler.get_autocorr_time; with autocorr='device' from the chain on the device (msx_series_acf).
        Rows the device holds past len(self._chain) -- queued chunks not consumed yet -- are not part of it."""
        return self._stored().autocorr_time(0, quiet, c, tol, discard, thin)

    def get_summary(self, q=(0.16, 0.5, 0.84), discard=0, thin=1, cols=None):
        """The posterior summary of the stored chain, flattened over the walkers: {'count': N, 'min', 'max' (ncols,),
        'quantiles' (ncols, len(q))} -- ``np.quantile(get_chain(discard=, thin=, flat=True), q, axis=0).T`` exactly, from
        elements the device selects (mcmc_spec_amd.summary).  With autocorr='device' from the chain
        held there (rows past len(self._chain) -- queued chunks not consumed yet -- are not part of it); otherwise the
        host chain is uploaded first.  ``cols``: coordinates or ``summary.col_ratio(a, b)``; None for all coordinates."""
        return self._stored().summary(0, q, discard, thin, cols)

    def get_products(self, cols, q=(0.16, 0.5, 0.84), discard=0, thin=1, indices=None):
        """``get_summary``'s dict over DERIVED columns of the stored chain (``mcmc_spec_amd.products``: names such as
        'kep_contrast', 'pri_corr', 'sec_corr', or codes): every sample of ``get_chain(discard=, thin=, flat=True)`` goes
        through the products kernel -- with autocorr='device' the chain held on the device, without a copy; otherwise the
        host chain is uploaded first -- and the device selects the order statistics.  ``indices``: positions in that flat
        sample to use instead of all of it (the reference draws 2,000 with ``np.random.choice(len(sample), 2000,
        replace=False)``, mft6.py:2486; the caller draws them): those samples are taken from the host copy of the chain
        and go through msx_products_batch, whatever ``autocorr`` is.  The engine needs staged products (``products.stage``)."""
        return self._stored().products(cols, 0, q, discard, thin, None if indices is None else [indices])

    def get_predictive(self, q=(0.16, 0.5, 0.84), discard=0, thin=1):
        """The posterior predictive check of the stored chain (``mcmc_spec_amd.predictive``): every
        sample of ``get_chain(discard=, thin=, flat=True)`` goes through the model once more and is reduced per data pixel
        on the device -- ``predictive.check``'s dict (``worst_status`` in place of ``terms`` and ``status``).  With
        autocorr='device' the chain held on the device is read, without a copy (rows past len(self._chain) -- queued chunks
        not consumed yet -- are not part of it); otherwise the host chain is uploaded first.  The engine needs staged
        products (``products.stage``)."""
        return self._stored().predictive(0, q, discard, thin)

    def get_loo(self, discard=0, thin=1, reff=1.0):
        """PSIS-LOO, WAIC and khat per observation of the stored chain (``mcmc_spec_amd.psis``):
        ``psis.loo``'s dict (``worst_status`` in place of ``status``) over ``get_chain(discard=, thin=, flat=True)``, from
        the chain held on the device with autocorr='device', otherwise from the host chain uploaded first.  A relative score
        between models on identical data (``psis.compare``), and the observations one sample cannot stand in for (khat >
        0.7).  The engine needs staged products (``products.stage``)."""
        return self._stored().loo(0, discard, thin, reff)

    def get_reweighted(self, engines_new, mode='logposterior', discard=0, thin=1):
        """The stored chain asked another question without a second run (``mcmc_spec_amd.reweight``):
        a ``reweight.Reweighted`` whose log-weight is ``lp_new - lp_old`` -- ``lp_new`` the ``mode`` of ``engines_new`` (one
        staged Engine: the same data under another prior, with ``rad_prior``, without the contrasts, ...), ``lp_old`` the
        sampler's own density under its own engine, both scored once more on the device.  Its ``stats['ess']`` says how far
        the second question is from the first; ``moments()`` and ``resample()`` answer it.  With autocorr='device' on the
        chain held there (rows past len(self._chain) are not part of it); otherwise the host chain is uploaded first.  The
        caller ``close()``s the result."""
        e_new = engines_new[0] if isinstance(engines_new, (list, tuple)) else engines_new
        return self._stored().reweighted([e_new], mode=mode, mode_old=self.mode, discard=discard, thin=thin)


def _autocorr_1d(x):
    x = np.asarray(x, dtype=float)
    n = 1 << int(np.ceil(np.log2(max(len(x), 2))))
    f = np.fft.fft(x - np.mean(x), n=2 * n)
    acf = np.fft.ifft(f * np.conjugate(f))[: len(x)].real
    if acf[0] == 0:
        return np.ones(len(x))
    return acf / acf[0]


class _Call:
    def __init__(self, f, args, kwargs):
        self.f, self.args, self.kwargs = f, args, kwargs

    def __call__(self, x):
        return self.f(x, *self.args, **self.kwargs)


def _max_rhat(get_rhat):
    """max over the columns of a check's split R-hat; NaN while the chain is shorter than 4 rows."""
    try:
        return float(np.max(get_rhat()))   # (np.max: a NaN column makes the maximum NaN, and NaN < rhat is False)
    except ValueError:
        return float('nan')


def run_reference_protocol(sampler, pos, nburn, nsteps, nthin=10, dirname=None, fname='run', rhat=None, ess=None):
    """The driver loop of ``run_emcee`` (mft6.py:1494-1529): burn-in, reset, production with the
    ``acl*50 < n`` / 10 % stability convergence test, thinned coordinate dumps and ``samples.txt``.
    Returns the flattened samples ``(nwalkers*nsteps_run, ndim)``.

    ``rhat`` (a float; None: the reference's rule alone, nothing else changes): a check stops only when
    ``max(sampler.get_rhat()) < rhat`` as well -- the second opinion that looks ACROSS the walkers, which tau cannot give
     -- and with ``dirname`` every check appends that maximum to ``{fname}_rhat.txt``.

    ``ess`` (a float; None: nothing changes): a check stops only when the smallest bulk and tail effective sample size over
    the columns (``sampler.get_ess``) has reached it as well, and with ``dirname`` every check appends
    that minimum to ``{fname}_ess.txt``."""
    import os
    for n, s in enumerate(sampler.sample(pos, iterations=nburn)):
        if dirname and n % nthin == 0:
            with open('{}/{}_{}_burnin.txt'.format(dirname, fname, n), 'ab') as f:
                f.write(b'\n')
                np.savetxt(f, s.coords)
    state = sampler.get_last_sample()
    sampler.reset()
    old_acl = np.inf
    for n, s in enumerate(sampler.sample(state, iterations=nsteps)):
        if n % nthin == 0:
            if dirname:
                with open('{}/{}_{}_results.txt'.format(dirname, fname, n), 'ab') as f:
                    f.write(b'\n')
                    np.savetxt(f, s.coords)
            acl = sampler.get_autocorr_time(quiet=True)
            macl = np.mean(acl)
            if dirname:
                with open('{}/{}_autocorr.txt'.format(dirname, fname), 'a') as f:
                    f.write(str(macl) + '\n')
            if rhat is not None:
                mrhat = _max_rhat(sampler.get_rhat)
                if dirname:
                    with open('{}/{}_rhat.txt'.format(dirname, fname), 'a') as f:
                        f.write(str(mrhat) + '\n')
            if ess is not None:
                mess = _min_ess(sampler)
                if dirname:
                    with open('{}/{}_ess.txt'.format(dirname, fname), 'a') as f:
                        f.write(str(mess) + '\n')
            if not np.isnan(macl):
                converged = np.all(acl * 50 < n)
                converged &= np.all((np.abs(old_acl - acl) / acl) < 0.1)
                if rhat is not None:
                    converged &= mrhat < rhat
                if ess is not None:
                    converged &= mess >= ess
                if converged:
                    break
            old_acl = acl
    samples = sampler.chain[:, :, :].reshape((-1, sampler.ndim))
    if dirname:
        np.savetxt(os.path.join(dirname, 'samples.txt'), samples)
    return samples
