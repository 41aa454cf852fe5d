"""CPU: every target's ladder stepped in lock-step on the host (mcmc_spec_amd.tempered.GroupTemperedSampler; DESIGN.md section
20) -- the definition a group's device run is pinned to.  Target k of the group is ``TemperedSampler`` on target k alone: the
chain, the densities, the counts, the last state and, adaptive, the ladders; across a reset, with unequal walker counts,
ladders and moves' streams per target, with two evaluation calls per half-step for ALL targets.  And what the sampler refuses."""
import numpy as np
import pytest

import common  # noqa: F401
from mcmc_spec_amd.moves import DEMove, StretchMove
from mcmc_spec_amd.tempered import DeviceGroupTemperedSampler, GroupTemperedSampler, TemperedSampler, TemperedState

NW = [12, 20, 8]
SEEDS = [21, 2**63 + 9, [5, 77, 1234]]
BETAS = [[1.0, 0.5, 0.25], [1.0, 0.3, 0.05], [1.0, 0.6, 0.2]]
NDIM = 3


def mix():
    return [(StretchMove(), 0.5), (DEMove(), 0.4), (DEMove(gamma0=1.0), 0.1)]


def two_modes(centre, width):
    """Two Gaussian modes at +-centre of unequal widths: the likelihood of an analytic bimodal target."""
    def ll(x):
        a = -0.5 * np.sum((x - centre) ** 2, axis=-1) / width ** 2
        b = -0.5 * np.sum((x + centre) ** 2, axis=-1) / (2.0 * width) ** 2 - NDIM * np.log(2.0)
        return np.logaddexp(a, b)
    return ll


def box(half):
    return lambda x: np.where(np.all(np.abs(x) < half, axis=-1), 0.0, -np.inf)


LIKES = [two_modes(1.0, 0.3), two_modes(1.5, 0.2), two_modes(0.7, 0.4)]
PRIORS = [box(3.0), box(2.5), box(4.0)]


class Batched:
    """K density functions as one batched call, counting the calls."""

    def __init__(self, fns):
        self.fns, self.calls = fns, 0

    def __call__(self, qs):
        self.calls += 1
        assert len(qs) == len(self.fns)
        return [f(np.asarray(q)) for f, q in zip(self.fns, qs)]


def starts():
    rng = np.random.default_rng(3)
    return [rng.uniform(-2.0, 2.0, size=(n, NDIM)) for n in NW]


def solo(k, **kw):
    seed, seeds = (SEEDS[k], None) if np.ndim(SEEDS[k]) == 0 else (None, SEEDS[k])
    return TemperedSampler(NW[k], NDIM, LIKES[k], PRIORS[k], betas=BETAS[k], seed=seed, seeds=seeds, moves=mix(), **kw)


def same(a, b):
    assert np.array_equal(a.get_chain(t=None), b.get_chain(t=None))
    assert np.array_equal(a.get_log_like(t=None), b.get_log_like(t=None)) and np.array_equal(a.get_log_prior(t=None), b.get_log_prior(t=None))
    assert np.array_equal(a.acceptance_fraction, b.acceptance_fraction) and np.array_equal(a.swap_fraction, b.swap_fraction)
    assert np.array_equal(a.get_betas(), b.get_betas()) and np.array_equal(a.betas, b.betas)
    la, lb = a.get_last_sample(), b.get_last_sample()
    assert np.array_equal(la.coords, lb.coords) and np.array_equal(la.log_like, lb.log_like) and np.array_equal(la.log_prior, lb.log_prior)


@pytest.mark.parametrize('adaptive', [False, True])
def test_target_k_of_the_group_is_the_tempered_sampler_on_target_k_alone(adaptive):
    kw = dict(adaptive=True, adaptation_lag=10.0, adaptation_time=1.0) if adaptive else {}
    ll, lpr = Batched(LIKES), Batched(PRIORS)
    g = GroupTemperedSampler(NW, NDIM, ll, lpr, betas=BETAS, seeds=SEEDS, moves=mix(), **kw)
    assert g.ntemps == 3 and g.nwalkers == NW and g.target(2).seeds == SEEDS[2] and g.target(0).seeds == [21, 22, 23]
    p0 = starts()
    st = g.run_mcmc(p0, 5)
    assert ll.calls == lpr.calls == 1 + 2 * 5                  # the start, then two calls per half-step for ALL targets
    assert len(st) == 3 and all(isinstance(s, TemperedState) for s in st)
    ones = [solo(k, **kw) for k in range(3)]
    st1 = [o.run_mcmc(p, 5) for o, p in zip(ones, p0)]
    for k in range(3):
        same(g.target(k), ones[k])
    assert not np.array_equal(g.target(0).get_chain()[:, :8], g.target(2).get_chain())
    g.reset()                                                   # the streams go on; a TemperedState needs no evaluation
    g.run_mcmc(st, 6)
    assert ll.calls == 1 + 2 * 11
    for k in range(3):
        ones[k].reset()
        ones[k].run_mcmc(st1[k], 6)
        same(g.target(k), ones[k])
        assert g.target(k).get_chain(t=None).shape == (6, 3, NW[k], NDIM)
        sw = g.target(k).swap_fraction
        assert np.all(sw > 0) and np.all(sw < 1)               # accepted and refused swaps both occur
    if adaptive:
        assert all(g.target(k)._adapted == 11 for k in range(3))
        assert not np.array_equal(g.target(0).betas, np.array(BETAS[0])) and g.target(0).betas[0] == 1.0 and g.target(0).betas[-1] == 0.25
        g.run_mcmc(g.run_mcmc(st, 1), 2, adapt=False)          # frozen: the rows repeat the ladder
        assert np.array_equal(g.target(1).get_betas()[-1], g.target(1).betas) and g.target(1)._adapted == 12
        with pytest.raises(ValueError, match='adapt=False'):
            g.target(1).log_evidence(blocks=2)
        assert np.isfinite(g.target(1).log_evidence(discard=7, blocks=2).log_z)


def test_one_ladder_for_all_targets_and_statuses_name_their_target():
    ll, lpr = Batched(LIKES), Batched(PRIORS)
    g = GroupTemperedSampler(NW, NDIM, ll, lpr, ntemps=4, beta_min=0.1, seeds=[1, 2, 3])
    assert all(np.array_equal(g.target(k).betas, np.geomspace(1.0, 0.1, 4)) for k in range(3))
    g.run_mcmc(starts(), 2)
    assert g.target(1).get_chain(t=3).shape == (2, NW[1], NDIM)
    # a likelihood that reports an error status on target 1 alone, where the prior admits the walker
    def bad(qs):
        out = [f(np.asarray(q)) for f, q in zip(LIKES, qs)]
        return [out[0], (out[1], np.full(len(out[1]), 4, dtype=np.int32)), out[2]]
    g = GroupTemperedSampler(NW, NDIM, bad, lpr, betas=BETAS, seeds=[1, 2, 3])
    with pytest.raises(Exception, match='^.?target 1: '):
        g.run_mcmc(starts(), 1)
    outside = starts()
    outside[2][3] = 100.0
    g = GroupTemperedSampler(NW, NDIM, ll, lpr, betas=BETAS, seeds=[1, 2, 3])
    with pytest.raises(ValueError, match='target 2: an initial walker lies outside the prior'):
        g.run_mcmc(outside, 1)


def test_what_the_samplers_refuse():
    ll, lpr = Batched(LIKES), Batched(PRIORS)
    with pytest.raises(ValueError, match='share ntemps'):
        GroupTemperedSampler(NW, NDIM, ll, lpr, betas=[[1.0, 0.5], [1.0, 0.5, 0.2], [1.0, 0.5]])
    with pytest.raises(ValueError, match='one ladder for all targets or one per target'):
        GroupTemperedSampler(NW, NDIM, ll, lpr, betas=BETAS[:2])
    with pytest.raises(ValueError, match='strictly descending'):
        GroupTemperedSampler(NW, NDIM, ll, lpr, betas=[BETAS[0], [1.0, 1.0, 0.5], BETAS[2]])
    with pytest.raises(ValueError, match='must not exceed 64'):
        GroupTemperedSampler(NW, NDIM, ll, lpr, ntemps=22)
    with pytest.raises(ValueError, match='seeds: one per target'):
        GroupTemperedSampler(NW, NDIM, ll, lpr, betas=BETAS, seeds=[1, 2])
    with pytest.raises(ValueError, match='even number'):
        GroupTemperedSampler([12, 7, 8], NDIM, ll, lpr, betas=BETAS)
    with pytest.raises(ValueError, match='adaptation_time'):
        GroupTemperedSampler(NW, NDIM, ll, lpr, betas=BETAS, adaptive=True, adaptation_time=[1.0, 0.5, 1.0])
    g = GroupTemperedSampler(NW, NDIM, ll, lpr, betas=BETAS)
    with pytest.raises(ValueError, match='one initial state per target'):
        g.run_mcmc(starts()[:2], 1)
    with pytest.raises(ValueError, match='target 1: incompatible input dimensions'):
        g.run_mcmc([starts()[0], starts()[0], starts()[2]], 1)

    class FakeGroup:   # (the device sampler checks its arguments before it touches a group)
        engines = [None] * 3

        def __len__(self):
            return 3
    for kw, msg in ((dict(rng='gpu'), "rng must be"), (dict(autocorr='gpu'), "autocorr must be"), (dict(chunk=0), 'chunk must be'),
                    (dict(ntemps=22), 'must not exceed 64')):
        with pytest.raises(ValueError, match=msg):
            DeviceGroupTemperedSampler(FakeGroup(), NW, NDIM, **dict(dict(betas=None if 'ntemps' in kw else BETAS), **kw))
    with pytest.raises(ValueError, match='one walker count per target'):
        DeviceGroupTemperedSampler(FakeGroup(), NW[:2], NDIM, betas=BETAS[:2])
