"""GPU: the target group's device-resident sampler (msx_group_sampler_*; mcmc_spec_amd.group.DeviceGroupSampler).  One
launch per half-step over every target's active half, the ensembles resident on the device: target k's chain must be bit
for bit the chain of GroupSampler on the same group and of target k's own EnsembleSampler with k's seed."""
import numpy as np
import pytest

from common import golden_case
from test_gpu_target_group import _stage, koi_engines, mixed_engines

pytestmark = pytest.mark.gpu


def spread(c, n, seed, scale=1.0):
    """n walkers around golden case c's first theta (tests/test_gpu_overlap.py's spread, any nspec)."""
    ns = c.nspec
    sc = np.array([30.0] * ns + [0.02] + [0.02] * ns + [2e-5]) * scale
    return c.theta[0] + np.random.default_rng(seed).normal(size=(n, 2 * ns + 2)) * sc


def check_against_group_and_solo(dev, host, engines, seeds, counts, p0s, n, mode):
    from mcmc_spec_amd.sampler import EnsembleSampler
    for k, eng in enumerate(engines):
        assert dev.get_chain(k).shape == (n, counts[k], p0s[k].shape[1])
        assert np.array_equal(dev.get_chain(k), host.get_chain(k)), k
        assert np.array_equal(dev.get_log_prob(k), host.get_log_prob(k)), k
        assert np.array_equal(dev.acceptance_fraction[k], host.acceptance_fraction[k]), k
        fn = eng.logposterior if mode == 'logposterior' else eng.loglikelihood
        es = EnsembleSampler(counts[k], p0s[k].shape[1], fn, vectorize=True, seed=seeds[k])
        es.run_mcmc(p0s[k], n)
        assert np.array_equal(dev.get_chain(k), es.get_chain()), k
        assert np.array_equal(dev.get_log_prob(k), es.get_log_prob()), k
        assert np.array_equal(dev.acceptance_fraction[k], es.acceptance_fraction), k


def test_koi_targets_walk_their_own_chains():
    """Eight KOI targets x 50 walkers, 30 iterations in chunks of 8 (a ragged last chunk)."""
    from mcmc_spec_amd import synth
    from mcmc_spec_amd.group import DeviceGroupSampler, GroupSampler, TargetGroup
    g, tags, engines = koi_engines()
    members = engines[:8]
    c = golden_case('A')
    grp = TargetGroup(members)
    K, n = len(members), 30
    counts = [50] * K
    seeds = [101 + k for k in range(K)]
    p0s = [synth.draw_walkers(50, seed=70 + k, tmin=c.tmin, tmax=c.tmax) for k in range(K)]
    dev = DeviceGroupSampler(counts, 6, grp, seeds=seeds, chunk=8)
    dev.run_mcmc(p0s, n)
    host = GroupSampler(counts, 6, grp.logposterior, seeds=seeds)
    host.run_mcmc(p0s, n)
    check_against_group_and_solo(dev, host, members, seeds, counts, p0s, n, 'logposterior')
    assert np.mean([a.mean() for a in dev.acceptance_fraction]) > 0.05
    grp.close()


@pytest.mark.parametrize('which', ['B', 'C'])
@pytest.mark.parametrize('mode', ['logposterior', 'loglikelihood'])
def test_mixed_members_and_unequal_walker_counts(which, mode):
    """Binaries / triples, crops, dist_fit / use_av off, rotated component grids; 16, 24, 50 and 512 walkers."""
    from mcmc_spec_amd.group import DeviceGroupSampler, GroupSampler, TargetGroup
    c, engines = mixed_engines(which)
    members = engines[:5] + engines[6:]   # (not the grid missing a node: walkers near it end in KeyError, by design)
    K, ndim, n = len(members), 2 * c.nspec + 2, 7
    counts = [(16, 24, 50, 512)[k % 4] for k in range(K)]
    seeds = [300 + k for k in range(K)]
    # (likelihood mode has no prior box: a step off the isochrone table or the grid is an error, not a rejection -- a
    # tighter ensemble keeps its few iterations on them)
    p0s = [spread(c, counts[k], 500 + k, 1.0 if mode == 'logposterior' else 0.1) for k in range(K)]
    if mode == 'loglikelihood':   # (and the companions 100 K above the table's lower end)
        for p in p0s:
            p[:, 1:c.nspec] += 100.0
    grp = TargetGroup(members)
    fn = grp.logposterior if mode == 'logposterior' else grp.loglikelihood
    dev = DeviceGroupSampler(counts, ndim, grp, mode=mode, seeds=seeds, chunk=3)
    dev.run_mcmc(p0s, n)
    host = GroupSampler(counts, ndim, fn, seeds=seeds)
    host.run_mcmc(p0s, n)
    check_against_group_and_solo(dev, host, members, seeds, counts, p0s, n, mode)
    grp.close()


def test_consecutive_runs_continue_the_chain():
    """run_mcmc(p0, n1) then run_mcmc(state, n2) = one GroupSampler run of n1 + n2; States with and without their
    log-probabilities give the same chain."""
    from mcmc_spec_amd.group import DeviceGroupSampler, GroupSampler, TargetGroup
    from mcmc_spec_amd.sampler import State
    c, engines = mixed_engines('B')
    members = engines[:3]
    grp = TargetGroup(members)
    counts, seeds = [16, 24, 50], [7, 8, 9]
    p0s = [spread(c, n, 40 + k) for k, n in enumerate(counts)]
    host = GroupSampler(counts, 6, grp.logposterior, seeds=seeds)
    host.run_mcmc(p0s, 11)
    dev = DeviceGroupSampler(counts, 6, grp, seeds=seeds, chunk=4)
    st = dev.run_mcmc(p0s, 5)
    dev.run_mcmc(st, 6)
    bare = DeviceGroupSampler(counts, 6, grp, seeds=seeds, chunk=4)
    st = bare.run_mcmc(p0s, 5)
    bare.run_mcmc([State(s.coords, np.empty(0)) for s in st], 6)   # (log-probabilities computed again: one launch)
    for k in range(3):
        for s in (dev, bare):
            assert np.array_equal(s.get_chain(k), host.get_chain(k)), k
            assert np.array_equal(s.get_log_prob(k), host.get_log_prob(k)), k
            assert np.array_equal(s.acceptance_fraction[k], host.acceptance_fraction[k]), k
    grp.close()


def test_a_walker_error_names_its_target():
    """Likelihood mode has no prior box: stretch moves below the isochrone table (2,900 K) are an error status.  Only
    target 1 starts there; the error is reported for target 1."""
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    c = golden_case('B')
    members = []
    for _ in range(3):
        e = Engine(0)
        e.stage_specs(c.specs)
        _stage(e, c, rad_prior=False)
        members.append(e)
    nw = 48
    p0s = [spread(c, nw, 9 + k) for k in range(3)]
    for k in (0, 2):   # the other targets' secondaries well inside the isochrone table
        p0s[k][:, 1] = 3300.0 + np.random.default_rng(k).normal(size=nw) * 3
    p0s[1][:, 1] = 2905.0 + np.abs(np.random.default_rng(2).normal(size=nw)) * 3
    grp = TargetGroup(members)
    s = DeviceGroupSampler([nw] * 3, 6, grp, mode='loglikelihood', seeds=[2, 3, 4], chunk=16)
    with pytest.raises(ValueError, match='target 1: '):
        s.run_mcmc(p0s, 60)
    # the chain up to the last collected chunk stands (chunks of 8, then 16)
    assert len({len(s.get_chain(k)) for k in range(3)}) == 1 and len(s.get_chain(1)) in (0, 8, 24, 40)
    grp.close()


def test_refusals():
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    from mcmc_spec_amd.sampler import EnsembleSampler
    c = golden_case('B')
    a, b = Engine(0), Engine(0)
    for e in (a, b):
        e.stage_specs(c.specs)
        _stage(e, c)
    grp = TargetGroup([a, b])
    g = grp.group
    p0 = spread(c, 32, 1)
    lp = np.concatenate(grp.logposterior([p0[:16], p0[16:]]))
    # the Python layer keeps EnsembleSampler's rule; the library refuses odd or too small counts itself
    with pytest.raises(ValueError, match='even number'):
        DeviceGroupSampler([16, 15], 6, grp)
    with pytest.raises(_lib.MsxError, match='member 1 has 15 walkers'):
        g.sampler_begin(_lib.MODE_LOGPOST, p0[:31], lp[:31], [16, 15], 4)
    with pytest.raises(_lib.MsxError, match='member 0 has 0 walkers'):
        g.sampler_begin(_lib.MODE_LOGPOST, p0[:16], lp[:16], [0, 16], 4)
    with pytest.raises(_lib.MsxError, match="P0 doesn't match"):
        g.sampler_begin(_lib.MODE_LOGPOST, np.zeros((32, 8)), lp, [16, 16], 4)
    # a member restaged mid-run: the next chunk is refused, then only end
    g.sampler_begin(_lib.MODE_LOGPOST, p0, lp, [16, 16], 4)
    es = [EnsembleSampler(16, 6, None, seed=s) for s in (1, 2)]

    def chunk(m):
        parts = [e._draw_split(m) + e._draw_moves(m) for e in es]
        return [np.concatenate(x, axis=2) for x in zip(*parts)]
    bad = chunk(2)
    bad[2] = bad[2].copy()
    bad[2][0, 0, 3] = 8   # partner index of member 0 past its half (8 walkers)
    with pytest.raises(_lib.MsxError, match='out of range'):
        g.sampler_enqueue(0, *bad)
    g.sampler_enqueue(0, *chunk(2))
    chain, lpc, nacc, worst = g.sampler_collect(0, 2)
    assert chain.shape == (2, 32, 6) and worst.shape == (2,) and not worst.any()
    _stage(b, c)
    with pytest.raises(_lib.MsxError, match='member 1.*staged again'):
        g.sampler_enqueue(1, *chunk(2))
    with pytest.raises(_lib.MsxError, match='failed'):
        g.sampler_enqueue(1, *chunk(2))
    with pytest.raises(_lib.MsxError, match='failed'):
        g.sampler_collect(0, 2)
    g.sampler_end()
    with pytest.raises(_lib.MsxError, match='begin first'):
        g.sampler_collect(0, 2)
    grp.close()
    # a destroyed member: refused at begin; a group destroyed with a run open ends it
    grp = TargetGroup([a, b])
    grp.group.sampler_begin(_lib.MODE_LOGPOST, p0, lp, [16, 16], 4)
    grp.close()
    grp = TargetGroup([a, b])
    a.ctx.close()
    with pytest.raises(_lib.MsxError, match='member 0 was destroyed'):
        grp.group.sampler_begin(_lib.MODE_LOGPOST, p0, lp, [16, 16], 4)
    grp.close()
