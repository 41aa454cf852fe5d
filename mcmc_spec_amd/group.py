"""Target groups: several staged targets evaluated in one launch, and a sampler that steps their ensembles together.

``TargetGroup(engines)`` wraps ``msx_group`` (include/msx.h): each ``Engine`` keeps its own grid and problem -- data,
bands, priors and grid may all differ, ``nspec`` must not -- and one launch evaluates every target's walkers, one
workgroup per walker, each against its own target.  Walker i of target k gets the bits ``engines[k]`` gives it alone.

``GroupSampler`` runs K stretch-move ensembles in lock-step from the host: per half-step, every target's proposals go
through ONE batched call ``f(list_of_thetas) -> list_of_logp`` (``TargetGroup.logposterior``: one launch).  Each target
draws its randomness from its own ``EnsembleSampler`` state, so target k's chain is bit for bit the chain of
``EnsembleSampler(nwalkers[k], ndim, f_k, vectorize=True, seed=seeds[k])`` run alone.

``DeviceGroupSampler`` walks the same chains with the ensembles resident on the GPU (``msx_group_sampler_*``): one launch
per half-step, no host round trip between half-steps, chunks of iterations queued back to back.
"""
from __future__ import annotations

from contextlib import closing

import numpy as np

from . import _lib
from .engine import _raise_for_status
from .sampler import EnsembleSampler, State, _accept, _max_rhat, _propose, _pump, device_seed
from .stored import StoredChain


class TargetGroup:
    """The walkers of several staged ``Engine``s in one launch.  ``thetas`` is a sequence of K arrays ``(nw_k, ndim)``
    (``nw_k`` may be 0); results are a list of K arrays.  The engines must stay open and staged: a target staged again,
    or closed, makes the group refuse every launch (create a new one)."""

    def __init__(self, engines):
        self.engines = list(engines)
        if not self.engines:
            raise ValueError('TargetGroup: at least one engine')
        for k, e in enumerate(self.engines):
            if e.tables is None:
                raise RuntimeError('TargetGroup: target {} has no staged problem'.format(k))
        self.ndim = self.engines[0].ndim
        self.group = _lib.Group([e.ctx for e in self.engines])

    def __len__(self):
        return len(self.engines)

    def _stack(self, thetas):
        if len(thetas) != len(self.engines):
            raise ValueError('one array of walkers per target ({} given, {} targets)'.format(len(thetas), len(self.engines)))
        arrs = []
        for t in thetas:
            a = np.asarray(t, dtype=float).reshape(-1, self.ndim) if np.size(t) == 0 else np.asarray(t, dtype=float)
            if a.ndim != 2 or a.shape[1] != self.ndim:
                raise ValueError("P0 doesn't match what I was expecting")  # (Engine's message, mft6.py:1457)
            arrs.append(a)
        counts = np.array([a.shape[0] for a in arrs], dtype=np.int64)
        theta = np.concatenate(arrs) if counts.sum() else np.empty((0, self.ndim))
        return arrs, counts, theta

    def _eval(self, thetas, mode):
        arrs, counts, theta = self._stack(thetas)
        if theta.shape[0] == 0:
            return [np.empty(0) for _ in arrs]
        logp, status = self.group.logprob_batch(theta, counts, mode)
        out, o = [], 0
        for k, a in enumerate(arrs):
            st = status[o:o + len(a)]
            try:
                _raise_for_status(st, a)
            except (KeyError, IndexError, ValueError, RuntimeError) as e:
                raise type(e)('target {}: {}'.format(k, e.args[0] if e.args else e)) from None
            out.append(logp[o:o + len(a)].copy())
            o += len(a)
        return out

    def logposterior(self, thetas):
        return self._eval(thetas, _lib.MODE_LOGPOST)

    def logprior(self, thetas):
        return self._eval(thetas, _lib.MODE_LOGPRIOR)

    def loglikelihood(self, thetas, optimize=False):
        return self._eval(thetas, _lib.MODE_CHISQ if optimize else _lib.MODE_LOGLIKE)

    def launch_info(self, counts, mode=_lib.MODE_LOGPOST, block_threads=0):
        """What one launch of ``counts[k]`` walkers of target k would take (kernel, resources, workgroups)."""
        return self.group.launch_info(counts, mode, block_threads)

    def close(self):
        self.group.close()


class GroupSampler:
    """K stretch-move ensembles stepped in lock-step, one batched call per half-step.

    ``nwalkers`` and ``seeds``: one entry per target.  ``log_prob_fn(list_of_thetas) -> list_of_logp`` evaluates K arrays
    ``(n_k, ndim)`` at once (``TargetGroup.logposterior``, or any host function for tests).  ``draws`` (optional): one
    ``draws(first_iteration, m)`` callable per target, handed to the target's ``EnsembleSampler(draws=...)`` in place of its
    generators -- with ``ctx.sampler_draw`` of target k's device seed, the host twin of ``DeviceGroupSampler(rng='device')``."""

    def __init__(self, nwalkers, ndim, log_prob_fn, a=None, seeds=None, draws=None, moves=None, _general=False):
        """``moves``: ``EnsembleSampler``'s, one set for every target (each target chooses its own move per iteration from
        its own stream)."""
        nwalkers = [int(n) for n in nwalkers]
        seeds = [None] * len(nwalkers) if seeds is None else list(seeds)
        if len(seeds) != len(nwalkers):
            raise ValueError('one seed per target')
        draws = [None] * len(nwalkers) if draws is None else list(draws)
        if len(draws) != len(nwalkers):
            raise ValueError('one draws callable per target')
        self.ndim = int(ndim)
        self.log_prob_fn = log_prob_fn
        # one EnsembleSampler per target holds its generators and its bookkeeping; its own log_prob_fn is never called
        self.samplers = [EnsembleSampler(n, ndim, None, a=a, vectorize=True, seed=s, draws=d, moves=moves, _general=_general)
                         for n, s, d in zip(nwalkers, seeds, draws)]
        self._moves = self.samplers[0]._moves if self.samplers else None

    @property
    def nwalkers(self):
        return [s.nwalkers for s in self.samplers]

    def reset(self):
        for s in self.samplers:
            s.reset()

    def compute_log_prob(self, coords):
        """``log_prob_fn`` over K arrays, with ``EnsembleSampler.compute_log_prob``'s checks per target."""
        coords = [np.asarray(c, dtype=float) for c in coords]
        for c in coords:
            if np.any(~np.isfinite(c)):
                raise ValueError('At least one parameter value was infinite or NaN')
        lps = self.log_prob_fn(coords)
        if len(lps) != len(coords):
            raise ValueError('log_prob_fn returned the wrong number of targets')
        out = []
        for c, lp in zip(coords, lps):
            lp = np.asarray(lp, dtype=float)
            if lp.shape != (len(c),):
                raise ValueError('log_prob_fn returned the wrong shape')
            if np.any(np.isnan(lp)):
                raise ValueError('Probability function returned NaN')
            out.append(lp)
        return out

    def _stretch_step(self, coords, logp):
        """One iteration of every target: the move's half-steps (_propose, _accept), the K targets' evaluations batched."""
        draws = [s._draw_steps(1) for s in self.samplers]
        accepted = [np.zeros(s.nwalkers, dtype=bool) for s in self.samplers]
        for h in (0, 1):
            qs = [_propose(coords[k], d, h) for k, d in enumerate(draws)]
            for k, (d, q, new_lp) in enumerate(zip(draws, qs, self.compute_log_prob(qs))):
                _accept(coords[k], logp[k], accepted[k], d, h, q, new_lp)
        return accepted

    def _initial(self, initial_states):
        """Coordinates and log-probabilities per target from one State or coordinate array per target.  The targets that
        come without their log-probabilities are evaluated in one batched call of K arrays, the others' left empty."""
        if len(initial_states) != len(self.samplers):
            raise ValueError('one initial state per target')
        coords, logp = [], []
        for k, (st, smp) in enumerate(zip(initial_states, self.samplers)):
            if isinstance(st, State):
                c, lp = st.coords.copy(), st.log_prob.copy()
            else:
                c, lp = np.array(st, dtype=float), None
            if c.shape != (smp.nwalkers, self.ndim):
                raise ValueError('incompatible input dimensions (target {})'.format(k))
            coords.append(c)
            logp.append(lp if lp is not None and lp.shape == (smp.nwalkers,) else None)
        missing = [k for k, lp in enumerate(logp) if lp is None]
        if missing:
            lps = self.compute_log_prob([coords[k] if logp[k] is None else np.empty((0, self.ndim)) for k in range(len(coords))])
            for k in missing:
                logp[k] = lps[k]
        return coords, logp

    def sample(self, initial_states, iterations=1, store=True):
        """``initial_states``: one State or coordinate array ``(nwalkers[k], ndim)`` per target.  Yields a list of K States
        per iteration."""
        coords, logp = self._initial(initial_states)
        for _ in range(int(iterations)):
            acc = self._stretch_step(coords, logp)
            states = []
            for k, smp in enumerate(self.samplers):
                smp._accepted += acc[k]
                smp.iteration += 1
                if store:
                    smp._chain.append(coords[k].copy())
                    smp._logp.append(logp[k].copy())
                smp._last = State(coords[k], logp[k])
                states.append(smp._last)
            yield states

    def run_mcmc(self, initial_states, nsteps, **kw):
        st = None
        for st in self.sample(initial_states, iterations=nsteps, **kw):
            pass
        return st

    def get_chain(self, k, **kw):
        """Target k's chain, (nsteps, nwalkers[k], ndim) (``EnsembleSampler.get_chain``'s keywords)."""
        return self.samplers[k].get_chain(**kw)

    def get_log_prob(self, k, **kw):
        return self.samplers[k].get_log_prob(**kw)

    @property
    def acceptance_fraction(self):
        """One array per target."""
        return [s.acceptance_fraction for s in self.samplers]

    # ---- the analyses: the stored-chain view's, the targets as its members (mcmc_spec_amd.stored) ----
    def _host_members(self, members=None):
        """The targets' stored chains side by side, (n, sum of the walkers, ndim); ``members``: those targets' alone."""
        chains = [np.array(self.samplers[k]._chain) for k in (range(len(self.samplers)) if members is None else members)]
        return chains[0] if len(chains) == 1 and members is not None else np.concatenate(chains, axis=1)

    def _stored(self):
        return StoredChain(None, self._host_members, len(self.samplers[0]._chain), self.ndim, self.nwalkers)

    def get_autocorr_time(self, k=None, quiet=False, c=5.0, tol=50.0, discard=0, thin=1):
        """Target k's integrated autocorrelation time (ndim,), or every target's (K, ndim) for k None: each from the
        target's own walkers (EnsembleSampler.get_autocorr_time's keywords and rules)."""
        return self._stored().autocorr_time(k, quiet, c, tol, discard, thin)

    def get_rhat(self, k=None, discard=0, thin=1, cols=None):
        """Target k's split R-hat (ncols,), or every target's (K, ncols) for k None: each over the target's own walkers
        (EnsembleSampler.get_rhat's keywords and rules).  DeviceGroupSampler with autocorr='device':
        every target's from the chains on the device, ONE msx_series_moments call over all targets (rows queued past the
        stored chains are not part of it)."""
        return self._stored().moments(k, discard, thin, cols, False)['rhat']

    def get_moments(self, k=None, discard=0, thin=1, cols=None):
        """Target k's {'mean', 'cov', 'count'} (EnsembleSampler.get_moments), or every target's for k None: the arrays
        with a leading axis K.  DeviceGroupSampler with autocorr='device': from the chains on the device (get_rhat's rules)."""
        out = self._stored().moments(k, discard, thin, cols, rhat=False)
        return {name: out[name] for name in ('mean', 'cov', 'count')}

    def get_rank_rhat(self, k=None, discard=0, thin=1, cols=None):
        """Target k's {'bulk', 'folded', 'rhat'} (EnsembleSampler.get_rank_rhat), or every target's for
        k None: the arrays with a leading axis K."""
        return self._stored().rank_rhat(k, discard, thin, cols)

    def get_ess(self, k=None, discard=0, thin=1, cols=None, kind='bulk'):
        """Target k's effective sample size (ncols,) (EnsembleSampler.get_ess), or every target's (K, ncols) for k None."""
        return self._stored().ess(k, discard, thin, cols, kind)

    def get_mcse(self, k=None, discard=0, thin=1, cols=None, q=(0.16, 0.5, 0.84)):
        """Target k's {'mean', 'quantiles'} (EnsembleSampler.get_mcse), or every target's for k None."""
        return self._stored().mcse(k, discard, thin, cols, q)

    def get_modes(self, k=None, ncomp=2, discard=0, thin=1, cols=None, **fit_kw):
        """Every target's posterior modes (EnsembleSampler.get_modes: a ``modes.ModeFit`` with one member per target), or
        target k's alone (the same object cut to that member).  DeviceGroupSampler fits on the device, every target's EM jobs
        in ONE msx_series_modes call: with autocorr='device' on the chains held there, otherwise the host chains are uploaded
        first (DeviceEnsembleSampler.get_modes' rules)."""
        return self._stored().modes(k, ncomp, discard, thin, cols, **fit_kw)


class DeviceGroupSampler(GroupSampler):
    """``GroupSampler`` with the K ensembles resident in HBM (``msx_group_sampler_*``, include/msx.h): ``chunk`` iterations
    are queued on the GPU back to back, ONE launch of the group kernel per half-step over the active half of every
    target's ensemble, and only the chains come back.

    ``rng='host'`` (default): each target's randomness is drawn on the host by its own ``EnsembleSampler``'s generators, the
    calls ``GroupSampler`` makes, so target k's chain is bit for bit the chain of ``GroupSampler`` and of
    ``EnsembleSampler(nwalkers[k], ndim, f_k, vectorize=True, seed=seeds[k])``.  ``rng='device'``: the library draws every
    chunk on the GPU (``msx_group_sampler_enqueue_drawn``: one launch per chunk, nothing drawn, concatenated or uploaded by
    the host), target k from ``device_seeds[k]`` -- ``seeds[k]`` as ``DeviceEnsembleSampler.device_seed`` derives it -- and
    the ABSOLUTE iteration number, which every chunk queued advances and ``reset()`` leaves alone
    (``self.samplers[k]._drawn``, as ``EnsembleSampler(draws=...)`` counts on the host).  Target k's chain is then the one
    ``EnsembleSampler(draws=lambda i, m: ctx.sampler_draw(device_seeds[k], a, i, m, nwalkers[k], ndim))`` walks, and
    ``GroupSampler(draws=[...])`` with those callables.  Up to 4096 walkers per target.

    ``group`` is a ``TargetGroup``; ``mode`` ``'logposterior'`` or ``'loglikelihood'``.  Drawing chunk i+1 overlaps chunk i
    on the GPU (``DeviceEnsembleSampler``'s chunk pipeline, ``sampler._pump``); consecutive ``sample`` calls continue the
    generators.  A walker error raises what ``TargetGroup`` raises, prefixed ``target k:``; the run ends there and the
    chain up to the last collected chunk stands.

    With ``rng='device'`` the stream position counts iterations QUEUED, not consumed: a ``sample()`` loop left early (a
    ``break``, as ``run_group_protocol`` does once every target has converged, or a walker error) leaves ``_drawn`` past the
    last iteration yielded -- by the chunks already queued -- while the host twin ``GroupSampler(draws=...)`` stops at the
    last iteration it stepped.  Both remain valid chains; a later run on the same sampler then no longer matches the twin
    number for number."""

    DEVICE_RNG_MAX_WALKERS = 4096   # csrc/logprob_kernel.h, kDrawMaxWalkers: one ensemble's (key, index) sort in LDS

    def __init__(self, nwalkers, ndim, group, mode='logposterior', a=None, seeds=None, chunk=64, autocorr='host', rng='host',
                 moves=None, _general=False):
        if mode not in ('logposterior', 'loglikelihood'):
            raise ValueError("mode must be 'logposterior' or 'loglikelihood'")
        if rng not in ('host', 'device'):
            raise ValueError("rng must be 'host' or 'device'")
        nwalkers = [int(n) for n in nwalkers]
        if rng == 'device':
            for k, n in enumerate(nwalkers):
                if n > self.DEVICE_RNG_MAX_WALKERS:
                    raise ValueError("rng='device' takes up to {} walkers per target (target {} has {})".format(
                        self.DEVICE_RNG_MAX_WALKERS, k, n))
        if len(nwalkers) != len(group):
            raise ValueError('one walker count per target ({} given, {} targets)'.format(len(nwalkers), len(group)))
        if int(chunk) < 1:
            raise ValueError('chunk must be at least 1')
        self.group = group
        self.mode = mode
        self._mode = {'logposterior': _lib.MODE_LOGPOST, 'loglikelihood': _lib.MODE_LOGLIKE}[mode]
        fn = group.logposterior if mode == 'logposterior' else group.loglikelihood
        if autocorr not in ('host', 'device'):
            raise ValueError("autocorr must be 'host' or 'device'")
        super().__init__(nwalkers, ndim, fn, a=a, seeds=seeds, moves=moves, _general=_general)
        self.chunk = int(chunk)
        self.rng_mode = rng
        seeds = [None] * len(nwalkers) if seeds is None else list(seeds)
        self.device_seeds = [device_seed(s) for s in seeds] if rng == 'device' else None
        # autocorr='device': the targets' stored chains are kept on the device too (one _lib.Series of K members, appended
        # by every sample(store=True) run) and get_autocorr_time computes all targets' autocorrelation there, one
        # msx_series_acf call per lag tile; 'host': GroupSampler's, per target
        self.autocorr = autocorr
        self._series = _lib.Series(group.engines[0].ctx, sum(nwalkers), self.ndim, nwalkers) if autocorr == 'device' else None

    def _draw_split_all(self, m):
        split = [s._draw_split(m) for s in self.samplers]
        return [np.concatenate(x, axis=2) for x in zip(*split)]

    def _draw_moves_all(self, m):
        moves = [s._draw_moves(m) for s in self.samplers]
        if self._moves is not None:   # the general layout: kind (m, K), the other arrays side by side
            return [np.stack([mv[0] for mv in moves], axis=1)] + [np.concatenate(x, axis=2) for x in list(zip(*moves))[1:]]
        return [np.concatenate(x, axis=2) for x in zip(*moves)]

    def _enqueue(self, slot, m, arrays):
        grp = self.group.group
        if arrays is not None:
            return (grp.sampler_enqueue_moves if self._moves is not None else grp.sampler_enqueue)(slot, *arrays)
        # the device draws: every target's stream at its absolute iteration (equal for all targets), which only a queued
        # chunk advances
        if self._moves is not None:
            grp.sampler_enqueue_moves_drawn(slot, m, self.device_seeds, self._moves, self.samplers[0]._drawn)
        else:
            grp.sampler_enqueue_drawn(slot, m, self.device_seeds, self.samplers[0].a, self.samplers[0]._drawn)
        for s in self.samplers:
            s._drawn += m
        return m

    def _chunks(self, coords, logp, iterations, store):
        """One run of ``iterations`` over the group: yields ``(m, chain, logp_chain, off)`` per collected chunk of m
        iterations -- rows [m][sum nwalkers] with target k's walkers at ``off[k]:off[k + 1]`` -- after raising the chunk's
        walker errors and setting every target's acceptance counts."""
        counts = self.nwalkers
        off = np.concatenate([[0], np.cumsum(counts)]).astype(int)
        grp = self.group.group
        base_acc = [s._accepted.copy() for s in self.samplers]
        grp.sampler_begin(self._mode, np.concatenate(coords), np.concatenate(logp), counts, self.chunk)
        if store and self._series is not None:
            try:
                grp.sampler_attach_series(self._series, len(self.samplers[0]._chain))
            except Exception:
                grp.sampler_end()
                raise
        draws = None if self.rng_mode == 'device' else (self._draw_split_all, self._draw_moves_all)
        with closing(_pump(iterations, self.chunk, draws, self._enqueue, grp.sampler_collect, grp.sampler_end)) as chunks:
            for mm, (chain, lpc, nacc, worst) in chunks:
                for k in np.nonzero(worst > _lib.W_REJECT)[0]:
                    try:
                        _raise_for_status(worst[k:k + 1], chain[-1, off[k]:off[k] + 1])
                    except (KeyError, IndexError, ValueError, RuntimeError) as e:
                        raise type(e)('target {}: {}'.format(k, e.args[0] if e.args else e)) from None
                for k, s in enumerate(self.samplers):
                    s._accepted = base_acc[k] + nacc[off[k]:off[k + 1]]
                yield mm, chain, lpc, off

    def sample(self, initial_states, iterations=1, store=True):
        """``initial_states``: one State or coordinate array ``(nwalkers[k], ndim)`` per target.  Yields a list of K States
        per iteration."""
        coords, logp = self._initial(initial_states)
        if int(iterations) <= 0:
            return
        with closing(self._chunks(coords, logp, iterations, store)) as chunks:
            for mm, chain, lpc, off in chunks:
                for i in range(mm):
                    states = []
                    for k, s in enumerate(self.samplers):
                        c, lp = chain[i, off[k]:off[k + 1]], lpc[i, off[k]:off[k + 1]]
                        s.iteration += 1
                        if store:
                            s._chain.append(c)
                            s._logp.append(lp)
                        s._last = State(c, lp)
                        states.append(s._last)
                    yield states

    def run_mcmc(self, initial_states, nsteps, store=True):
        """``sample`` consumed by whole chunks: each chunk's rows go to the targets' chains at once and the K States are
        built for the last iteration only (building K States per iteration is host time the GPU waits for: DESIGN.md
        section 11.2).  Chains, log-probabilities, acceptance counts and the returned States are those of
        ``for states in sample(initial_states, nsteps): pass``, bit for bit."""
        coords, logp = self._initial(initial_states)
        if int(nsteps) <= 0:
            return None
        last = None
        try:
            with closing(self._chunks(coords, logp, nsteps, store)) as chunks:
                for mm, chain, lpc, off in chunks:
                    for k, s in enumerate(self.samplers):
                        s.iteration += mm
                        if store:
                            s._chain.extend(chain[:, off[k]:off[k + 1]])
                            s._logp.extend(lpc[:, off[k]:off[k + 1]])
                    last = (chain[mm - 1], lpc[mm - 1], off)
        finally:   # (also when a chunk raised: the last collected iteration is every target's last sample, as in sample())
            if last is not None:
                c, lp, off = last
                for k, s in enumerate(self.samplers):
                    s._last = State(c[off[k]:off[k + 1]], lp[off[k]:off[k + 1]])
        return [s._last for s in self.samplers]

    def _stored(self):
        """GroupSampler's view with the resident series (autocorr='device'), the targets' engines, and the mode fit on the
        device (the targets step together: their chains have one length)."""
        return StoredChain(self._series, self._host_members, len(self.samplers[0]._chain), self.ndim, self.nwalkers,
                           self.group.engines, device_modes=True)

    def get_autocorr_time(self, k=None, quiet=False, c=5.0, tol=50.0, discard=0, thin=1):
        """GroupSampler.get_autocorr_time; with autocorr='device' every target's from the chains on the device, ONE
        msx_series_acf call per lag tile over all targets (the targets step together: their chains have one length)."""
        return self._stored().autocorr_time(k, quiet, c, tol, discard, thin)

    def get_summary(self, k=None, q=(0.16, 0.5, 0.84), discard=0, thin=1, cols=None):
        """Every target's posterior summary from its stored chain, flattened over its walkers: {'count' (K,), 'min', 'max'
        (K, ncols), 'quantiles' (K, ncols, len(q))}, ``np.quantile``'s numbers exactly; for one target with ``k`` (the
        arrays lose their first axis).  One set of device calls covers all targets (mcmc_spec_amd.summary; DESIGN.md
        section 14): with autocorr='device' on the chains held there -- the rows of the stored chains; rows queued past
        them are not part of it -- otherwise the host chains are uploaded first.  ``cols``: coordinates or
        ``summary.col_ratio(a, b)``; None for all coordinates."""
        return self._stored().summary(k, q, discard, thin, cols)

    def get_products(self, cols, q=(0.16, 0.5, 0.84), discard=0, thin=1, indices=None, k=None):
        """``get_summary``'s dict over DERIVED columns (``mcmc_spec_amd.products``) of every target's stored chain, each
        target's samples evaluated with its own engine's problem and products in one launch: with autocorr='device' on
        the chains held there, otherwise the host chains are uploaded first.  ``indices``: positions in each target's flat
        sample ``get_chain(k, discard=, thin=, flat=True)`` to use instead of all of it -- one index array for every
        target or a sequence of K (mft6.py:2486: the caller draws them); those samples are taken from the host copies of the
        chains and go through msx_products_batch target by target, whatever ``autocorr`` is.  ``k``: one target (the arrays lose their first
        axis).  Every engine needs staged products (``products.stage``)."""
        return self._stored().products(cols, k, q, discard, thin, indices)

    def get_predictive(self, q=(0.16, 0.5, 0.84), discard=0, thin=1, k=None):
        """Every target's posterior predictive check (``mcmc_spec_amd.predictive``) of its stored
        chain, each target's samples evaluated with its own engine: a list of K dicts (the targets' pixel counts may
        differ), or target ``k``'s dict.  With autocorr='device' on the chains held there, otherwise the host chains are
        uploaded first; rows queued past the stored chains are not part of it."""
        return self._stored().predictive(k, q, discard, thin)

    def get_loo(self, discard=0, thin=1, reff=1.0, k=None):
        """Every target's PSIS-LOO, WAIC and khat per observation (``mcmc_spec_amd.psis``) of its
        stored chain, each target's samples evaluated with its own engine: a list of K ``psis.loo`` dicts, or target
        ``k``'s.  With autocorr='device' on the chains held there, otherwise the host chains are uploaded first."""
        return self._stored().loo(k, discard, thin, reff)

    def get_reweighted(self, engines_new, mode='logposterior', discard=0, thin=1):
        """``DeviceEnsembleSampler.get_reweighted`` for every target at once: ``engines_new`` holds one staged Engine per
        target (a target's own engine leaves its weights at 1), and the ``reweight.Reweighted`` it returns has one member
        per target.  With autocorr='device' on the chains held there, otherwise the host chains are uploaded first."""
        engines_new = list(engines_new)
        if len(engines_new) != len(self.group.engines):
            raise ValueError('get_reweighted: one engine per target ({})'.format(len(self.group.engines)))
        return self._stored().reweighted(engines_new, mode=mode, mode_old=self.mode, discard=discard, thin=thin)


def run_group_protocol(sampler, pos, nburn, nsteps, nthin=10, dirname=None, fnames=None, rhat=None, ess=None):
    """``sampler.run_reference_protocol`` (run_emcee's driver, mft6.py:1494-1529) applied to every target of a group
    sampler (GroupSampler or DeviceGroupSampler) stepped in lock-step: burn-in, reset, then production with one tau
    computation for all targets every ``nthin`` iterations.  Each target keeps its own ``old_acl``; a target that meets
    ``acl * 50 < n`` and the 10 % rule is finished at that n -- its samples, its results dumps and its autocorr lines stop
    there -- and the group keeps stepping until every target has finished or ``nsteps`` runs out.

    ``pos``: one initial state per target.  ``dirname``: one directory per target (a sequence), or one directory under
    which target k writes into ``dirname/fnames[k]/``; ``fnames``: the targets' file prefixes (default ``run0``, ``run1``,
    ...).  Target k's files are those ``run_reference_protocol(dirname=<its directory>, fname=fnames[k])`` writes.
    Returns the K targets' flattened samples; target k's are exactly ``run_reference_protocol``'s on target k alone with
    k's seed (its chain in the group is its own chain, bit for bit).

    ``rhat`` (a float; None: nothing changes): ``run_reference_protocol``'s -- a target finishes at a check only when the
    maximum of its split R-hat lies below ``rhat`` as well, and with ``dirname`` every check appends that maximum to the
    target's ``{fname}_rhat.txt``.

    ``ess`` (a float; None: nothing changes): ``run_reference_protocol``'s -- a target finishes at a check only when the
    smallest of its bulk and tail effective sample sizes has reached ``ess`` as well, and with ``dirname`` every check
    appends that minimum to the target's ``{fname}_ess.txt``."""
    import os
    K, ndim = len(sampler.samplers), sampler.ndim
    fnames = ['run{}'.format(k) for k in range(K)] if fnames is None else [str(f) for f in fnames]
    if len(fnames) != K:
        raise ValueError('one file prefix per target')
    dirs = None
    if dirname is not None:
        if isinstance(dirname, (str, bytes, os.PathLike)):
            dirs = [os.path.join(dirname, f) for f in fnames]
            for d in dirs:
                os.makedirs(d, exist_ok=True)
        else:
            dirs = list(dirname)
            if len(dirs) != K:
                raise ValueError('one directory per target')

    def dump(k, what, coords):
        with open('{}/{}_{}.txt'.format(dirs[k], fnames[k], what), 'ab') as f:
            f.write(b'\n')
            np.savetxt(f, coords)

    for n, states in enumerate(sampler.sample(pos, iterations=nburn)):
        if dirs and n % nthin == 0:
            for k in range(K):
                dump(k, '{}_burnin'.format(n), states[k].coords)
    state = [s.get_last_sample() for s in sampler.samplers]
    sampler.reset()
    old_acl = [np.inf] * K
    stop = [None] * K   # the production iteration at which target k finished
    at_once = getattr(sampler, '_series', None) is not None
    for n, states in enumerate(sampler.sample(state, iterations=nsteps)):
        if n % nthin:
            continue
        active = [k for k in range(K) if stop[k] is None]
        if dirs:
            for k in active:
                dump(k, '{}_results'.format(n), states[k].coords)
        if at_once:   # (one device computation for all targets)
            acls = sampler.get_autocorr_time(quiet=True)
        else:
            acls = {k: sampler.get_autocorr_time(k, quiet=True) for k in active}
        if rhat is not None:
            if at_once:   # (one device computation for all targets; NaN while the chains are shorter than 4 rows)
                try:
                    mrhats = np.max(sampler.get_rhat(), axis=1)
                except ValueError:
                    mrhats = np.full(K, np.nan)
            else:
                mrhats = {k: _max_rhat(lambda: sampler.get_rhat(k)) for k in active}
        if ess is not None:   # (one computation for all targets; NaN while the chains are shorter than 4 rows)
            try:
                st = sampler._stored().rank_stats(None, ('bulk', 'tail'))
                messes = np.min(np.minimum(st['ess_bulk'], st['ess_tail']), axis=1)
            except ValueError:
                messes = np.full(K, np.nan)
        for k in active:
            acl = acls[k]
            macl = np.mean(acl)
            if dirs:
                with open('{}/{}_autocorr.txt'.format(dirs[k], fnames[k]), 'a') as f:
                    f.write(str(macl) + '\n')
                if rhat is not None:
                    with open('{}/{}_rhat.txt'.format(dirs[k], fnames[k]), 'a') as f:
                        f.write(str(float(mrhats[k])) + '\n')
                if ess is not None:
                    with open('{}/{}_ess.txt'.format(dirs[k], fnames[k]), 'a') as f:
                        f.write(str(float(messes[k])) + '\n')
            if not np.isnan(macl):
                converged = np.all(acl * 50 < n)
                converged &= np.all((np.abs(old_acl[k] - acl) / acl) < 0.1)
                if rhat is not None:
                    converged &= mrhats[k] < rhat
                if ess is not None:
                    converged &= messes[k] >= ess
                if converged:
                    stop[k] = n
                    continue
            old_acl[k] = acl
        if all(st is not None for st in stop):
            break
    out = []
    for k, s in enumerate(sampler.samplers):
        nk = len(s._chain) if stop[k] is None else stop[k] + 1
        samples = s.chain[:, :nk, :].reshape((-1, ndim))
        if dirs:
            np.savetxt(os.path.join(dirs[k], 'samples.txt'), samples)
        out.append(samples)
    return out
