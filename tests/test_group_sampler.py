"""CPU: GroupSampler (mcmc_spec_amd/group.py) steps K ensembles in lock-step through one batched call per half-step,
and target k's chain is bit for bit that of a separate EnsembleSampler with target k's walker count and seed."""
import numpy as np
import pytest

import common  # noqa: F401
from mcmc_spec_amd.group import GroupSampler
from mcmc_spec_amd.sampler import EnsembleSampler

NDIM = 6


def make_target(k):
    rng = np.random.default_rng(100 + k)
    mu, isig = rng.normal(size=NDIM), 1.0 / rng.uniform(0.5, 2.0, size=NDIM)

    def lnp(x):
        x = np.atleast_2d(x)
        return -0.5 * np.sum(((x - mu) * isig) ** 2, axis=1)
    return lnp


def never(x):  # every proposal rejected
    return np.full(len(np.atleast_2d(x)), -np.inf)


def run_both(fns, nws, seeds, iters, p0s):
    calls = []

    def batched(thetas):
        calls.append([len(t) for t in thetas])
        return [f(t) for f, t in zip(fns, thetas)]
    gs = GroupSampler(nws, NDIM, batched, seeds=seeds)
    gs.run_mcmc(p0s, iters)
    alone = []
    for f, nw, s, p0 in zip(fns, nws, seeds, p0s):
        es = EnsembleSampler(nw, NDIM, f, vectorize=True, seed=s)
        es.run_mcmc(p0, iters)
        alone.append(es)
    return gs, alone, calls


@pytest.mark.parametrize('nws', [[16, 16, 16], [12, 40, 20, 64]])
def test_lockstep_equals_separate_samplers(nws):
    fns = [make_target(k) for k in range(len(nws))]
    fns[1] = never  # a target whose proposals are all -inf
    seeds = [7 * k + 3 for k in range(len(nws))]
    p0s = [np.random.default_rng(k).normal(size=(nw, NDIM)) for k, nw in enumerate(nws)]
    gs, alone, calls = run_both(fns, nws, seeds, 25, p0s)
    # one call for the initial log-probabilities, then one per half-step, each carrying every target's half
    assert calls[0] == nws and len(calls) == 1 + 2 * 25
    assert all(c == [nw // 2 for nw in nws] for c in calls[1:])
    for k, es in enumerate(alone):
        assert np.array_equal(gs.get_chain(k), es.get_chain())
        assert np.array_equal(gs.get_log_prob(k), es.get_log_prob(), equal_nan=True)
        assert np.array_equal(gs.acceptance_fraction[k], es.acceptance_fraction)
    assert np.all(gs.acceptance_fraction[1] == 0.0)
    assert np.all(gs.get_chain(1) == p0s[1][None])
    assert gs.acceptance_fraction[0].mean() > 0.1


def test_resumes_from_states_like_the_separate_samplers():
    nws, seeds = [16, 24], [1, 2]
    fns = [make_target(0), make_target(1)]
    p0s = [np.random.default_rng(9 + k).normal(size=(nw, NDIM)) for k, nw in enumerate(nws)]
    gs = GroupSampler(nws, NDIM, lambda ts: [f(t) for f, t in zip(fns, ts)], seeds=seeds)
    st = gs.run_mcmc(p0s, 5)
    gs.reset()
    gs.run_mcmc(st, 7)
    for k in range(2):
        es = EnsembleSampler(nws[k], NDIM, fns[k], vectorize=True, seed=seeds[k])
        s = es.run_mcmc(p0s[k], 5)
        es.reset()
        es.run_mcmc(s, 7)
        assert np.array_equal(gs.get_chain(k), es.get_chain())


def test_nan_and_bad_shapes_raise():
    gs = GroupSampler([12, 12], NDIM, lambda ts: [np.full(len(t), np.nan) for t in ts], seeds=[0, 1])
    with pytest.raises(ValueError, match='NaN'):
        gs.run_mcmc([np.zeros((12, NDIM)), np.zeros((12, NDIM))], 1)
    with pytest.raises(ValueError, match='incompatible'):
        gs.run_mcmc([np.zeros((12, NDIM)), np.zeros((10, NDIM))], 1)
    with pytest.raises(ValueError):
        GroupSampler([12, 12], NDIM, None, seeds=[0])


def test_resumes_from_mixed_states_with_one_array_per_target():
    """Resumed from a State for some targets and bare coordinates for others: log_prob_fn still receives K arrays (the
    complete targets' empty), as TargetGroup.logposterior requires, and each target walks its EnsembleSampler chain."""
    nws, seeds = [12, 12, 16], [4, 5, 6]
    fns = [make_target(k) for k in range(3)]
    p0s = [np.random.default_rng(20 + k).normal(size=(nw, NDIM)) for k, nw in enumerate(nws)]
    calls = []

    def batched(thetas):
        if len(thetas) != len(fns):
            raise ValueError('one array of walkers per target')
        calls.append([len(t) for t in thetas])
        return [f(np.reshape(t, (-1, NDIM))) for f, t in zip(fns, thetas)]
    gs = GroupSampler(nws, NDIM, batched, seeds=seeds)
    st = gs.run_mcmc(p0s, 4)
    gs.reset()
    calls.clear()
    gs.run_mcmc([st[0], st[1].coords, st[2]], 6)
    assert calls[0] == [0, nws[1], 0]
    for k in range(3):
        es = EnsembleSampler(nws[k], NDIM, fns[k], vectorize=True, seed=seeds[k])
        s = es.run_mcmc(p0s[k], 4)
        es.reset()
        es.run_mcmc(s if k != 1 else s.coords, 6)
        assert np.array_equal(gs.get_chain(k), es.get_chain())
        assert np.array_equal(gs.get_log_prob(k), es.get_log_prob())
