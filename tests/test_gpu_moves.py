"""GPU: moves other than the stretch move and mixtures of moves on the device-resident samplers (include/msx.h,
msx_*_enqueue_moves*; csrc/move_kernels.h).  The path runs BESIDE the fused kernel -- a step kernel
proposes, the plain evaluation scores, the step kernel accepts -- so (a) a stretch-only set forced through it must walk the
default run's chain bit for bit, (b) a mixture must walk the chain of the host loop fed the device's own draws, (c) those
draws are the counter stream mcmc_spec_amd.moves.counter_draws_moves restates, (d) a target group's members walk their own
chains, (e) the device series and its summary see the same rows, and (f) the ABI refuses what it must."""
import numpy as np
import pytest

import common
from test_gpu_group_chain import spread
from test_gpu_overlap import _config2
from test_gpu_target_group import mixed_engines

pytestmark = pytest.mark.gpu

SEED = 17     # iterations 0..4 and 5..10 of this seed's stream each take all three moves of MIX (asserted below)
CHUNK = 4     # runs of 5 then 6 iterations: chunks are crossed and end short


def mix():
    from mcmc_spec_amd.moves import DEMove, StretchMove
    return [(StretchMove(), 0.5), (DEMove(), 0.4), (DEMove(gamma0=1.0), 0.1)]


def start(nw):
    from mcmc_spec_amd import synth
    eng, W = _config2()
    return eng, synth.draw_walkers(nw, seed=5 + nw, tmin=W['tmin'], tmax=W['tmax'])


def two_runs(s, p0):
    """5 iterations, reset(), 6 more from where the first run ended: (first run's chain, log-probs, acceptance), the sampler."""
    st = s.run_mcmc(p0, 5)
    first = (s.get_chain().copy(), s.get_log_prob().copy(), s.acceptance_fraction.copy(), st)
    s.reset()
    s.run_mcmc(st, 6)
    return first


def same_run(a, fa, b, fb):
    for x, y in zip(fa[:3], fb[:3]):
        assert np.array_equal(x, y)
    assert np.array_equal(fa[3].coords, fb[3].coords) and np.array_equal(fa[3].log_prob, fb[3].log_prob)
    assert a.get_chain().shape[0] == 6
    assert np.array_equal(a.get_chain(), b.get_chain()) and np.array_equal(a.get_log_prob(), b.get_log_prob())
    assert np.array_equal(a.acceptance_fraction, b.acceptance_fraction)
    la, lb = a.get_last_sample(), b.get_last_sample()
    assert np.array_equal(la.coords, lb.coords) and np.array_equal(la.log_prob, lb.log_prob)


# ---- (a) stretch through the general path equals the default run -------------------------------------------------------
@pytest.mark.parametrize('rng', ['host', 'device'])
@pytest.mark.parametrize('nw', [18, 256])
def test_stretch_through_the_general_path_is_the_default_run(nw, rng):
    """18 walkers: 9 per half, a fraction of a wave; 256: the size at which the default run overlaps its half-steps and
    this one must not."""
    from mcmc_spec_amd.moves import StretchMove
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    eng, p0 = start(nw)
    default = DeviceEnsembleSampler(nw, 6, eng, seed=SEED, chunk=CHUNK, rng=rng)
    fd = two_runs(default, p0)
    general = DeviceEnsembleSampler(nw, 6, eng, seed=SEED, chunk=CHUNK, rng=rng, moves=StretchMove(2.0), _general=True)
    assert general._moves is not None and default._moves is None
    fg = two_runs(general, p0)
    same_run(general, fg, default, fd)
    assert general.overlapped is False
    if nw == 256:
        assert default.overlapped is True
    assert 0.05 < general.acceptance_fraction.mean() < 0.95


# ---- (b) the mixture on the device equals the host twin ------------------------------------------------------------------
@pytest.mark.parametrize('nw', [18, 256])
def test_the_mixture_walks_the_host_twins_chain(nw):
    from mcmc_spec_amd.moves import counter_draws_moves
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler, EnsembleSampler
    eng, p0 = start(nw)
    kinds = counter_draws_moves(SEED, mix(), 6, 0, 11, nw)[2]
    which = eng.ctx.sampler_draw_moves(SEED, mix(), 0, 11, nw, 6)
    assert np.array_equal(which[2], kinds) and set(kinds[:5]) == {0, 1} == set(kinds[5:])
    # (every MOVE of the set, the jumping DE included: g = 1 up to sigma on its iterations)
    g = which[5]
    for rows in (slice(0, 5), slice(5, 11)):
        de = g[rows][kinds[rows] == 1]
        assert np.any(np.abs(de - 1.0) < 1e-3) and np.any(np.abs(de - 2.38 / np.sqrt(12.0)) < 1e-3)
    dev = DeviceEnsembleSampler(nw, 6, eng, seed=SEED, chunk=CHUNK, rng='device', moves=mix())
    fd = two_runs(dev, p0)
    host = EnsembleSampler(nw, 6, eng.logposterior, vectorize=True, moves=mix(),
                           draws=lambda i, m: eng.ctx.sampler_draw_moves(SEED, mix(), i, m, nw, 6))
    fh = two_runs(host, p0)
    same_run(dev, fd, host, fh)
    assert dev.overlapped is False and dev._drawn == 11 == host._drawn
    # accepted moves and rejected ones both occur (DE proposals that leave the prior box are rejected)
    acc = (fd[2] * 5).sum() + (dev.acceptance_fraction * 6).sum()
    print('acceptance fraction over the 11 iterations:', acc / (11 * nw))
    assert 0.02 < acc / (11 * nw) < 0.95
    fresh = DeviceEnsembleSampler(nw, 6, eng, seed=SEED, chunk=CHUNK, rng='device', moves=mix())   # (would replay iterations 0..5)
    fresh.run_mcmc(fd[3], 6)
    assert not np.array_equal(fresh.get_chain(), dev.get_chain())


def test_the_host_drawn_mixture_walks_the_host_loops_chain():
    """rng='host': the sampler's own NumPy generators, uploaded in the general layout (msx_sampler_enqueue_moves)."""
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler, EnsembleSampler
    eng, p0 = start(18)
    dev = DeviceEnsembleSampler(18, 6, eng, seed=SEED, chunk=CHUNK, moves=mix())
    fd = two_runs(dev, p0)
    host = EnsembleSampler(18, 6, eng.logposterior, vectorize=True, seed=SEED, moves=mix())
    fh = two_runs(host, p0)
    same_run(dev, fd, host, fh)
    assert dev.overlapped is False


# ---- (c) msx_sampler_draw_moves against the NumPy restatement -------------------------------------------------------------
@pytest.mark.parametrize('nw,ndim,seed', [(18, 6, 2**63 + 5), (256, 6, SEED), (2048, 8, 3)])
def test_the_device_draws_are_the_counter_stream_restated_in_numpy(nw, ndim, seed):
    from mcmc_spec_amd.moves import DEMove, counter_draws_moves
    eng, W = _config2()
    got = eng.ctx.sampler_draw_moves(seed, mix(), 0, 11, nw, ndim)
    want = counter_draws_moves(seed, mix(), ndim, 0, 11, nw)
    for i in (0, 1, 2, 3, 4):   # sidx, cidx, kind, p1, p2
        assert got[i].dtype == np.int32 and np.array_equal(got[i], want[i]), i
    kind = got[2]
    st, de = kind == 0, kind == 1
    assert st.any() and de.any()
    for i in (5, 6, 7):         # g = z, fac = (ndim - 1) ln z, logu on stretch entries
        assert np.allclose(got[i][st], want[i][st], rtol=4e-16, atol=1e-300), i
    assert np.array_equal(got[5][st], want[5][st])   # (z itself: no transcendental in it)
    assert np.allclose(got[5][de], want[5][de], rtol=1e-15, atol=0)
    assert np.all(got[6][de] == 0.0) and np.all(got[3][de] != got[4][de]) and np.array_equal(got[3][st], got[4][st])
    assert np.allclose(got[7][de], want[7][de], rtol=4e-16, atol=1e-300)
    # the split and u_z, u_p, u_a are the stretch-only generator's for the same seed
    plain = eng.ctx.sampler_draw(seed, 2.0, 0, 11, nw, ndim)
    assert np.array_equal(plain[0], got[0]) and np.array_equal(plain[1], got[1]) and np.array_equal(plain[5], got[7])
    assert np.array_equal(plain[2][st], got[3][st]) and np.array_equal(plain[3][st], got[5][st]) and np.array_equal(plain[4][st], got[6][st])
    # a later chunk is the stream's later rows
    later = eng.ctx.sampler_draw_moves(seed, mix(), 4, 7, nw, ndim)
    assert all(np.array_equal(a, b[4:]) for a, b in zip(later, got))
    # the normal deviate itself: g = 1 + n with sigma = gamma0 = 1.  1e-13 ABSOLUTE: the rounding of the argument 2 pi u2
    # moves cos by up to 7e-16, the radius is at most sqrt(-2 ln 2^-53) = 8.6 -- about 6e-15, with margin
    unit = DEMove(sigma=1.0, gamma0=1.0)
    gn, wn = eng.ctx.sampler_draw_moves(seed, unit, 0, 5, nw, ndim), counter_draws_moves(seed, unit, ndim, 0, 5, nw)
    assert np.all(gn[2] == 1) and np.array_equal(gn[3], wn[3]) and np.array_equal(gn[4], wn[4])
    n_dev, n_np = gn[5] - 1.0, wn[5] - 1.0
    print('normal deviate: max |device - numpy| =', np.abs(n_dev - n_np).max(), ' std', n_dev.std())
    assert np.abs(n_dev - n_np).max() <= 1e-13
    if nw >= 256:
        assert abs(n_dev.mean()) < 5.0 / np.sqrt(n_dev.size) and abs(n_dev.var() - 1.0) < 5.0 * np.sqrt(2.0 / n_dev.size)


# ---- (d) a target group ---------------------------------------------------------------------------------------------------
def group_same(dev, k, es):
    assert np.array_equal(dev.get_chain(k), es.get_chain()), k
    assert np.array_equal(dev.get_log_prob(k), es.get_log_prob()), k
    assert np.array_equal(dev.acceptance_fraction[k], es.acceptance_fraction), k


def group_case(case, counts, seeds, ndim, mode, scale):
    from mcmc_spec_amd.group import DeviceGroupSampler, GroupSampler, TargetGroup
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    c, engines = mixed_engines(case)
    members = engines[:len(counts)]
    p0s = [spread(c, counts[k], 500 + k, scale) for k in range(len(counts))]
    if case == 'C':   # (test_gpu_group_rng: the companions 100 K above the table's lower end)
        for p in p0s:
            p[:, 1:c.nspec] += 100.0
    grp = TargetGroup(members)
    fn = grp.logposterior if mode == 'logposterior' else grp.loglikelihood
    n = 7
    dev = DeviceGroupSampler(counts, ndim, grp, mode=mode, seeds=seeds, chunk=3, rng='device', moves=mix())
    dev.run_mcmc(p0s, n)
    draws = [(lambda i, m, k=k: members[k].ctx.sampler_draw_moves(seeds[k], mix(), i, m, counts[k], ndim)) for k in range(len(counts))]
    twin = GroupSampler(counts, ndim, fn, moves=mix(), draws=draws)
    twin.run_mcmc(p0s, n)
    kinds = set()
    for k, eng in enumerate(members):
        assert dev.get_chain(k).shape == (n, counts[k], ndim)
        group_same(dev, k, twin.samplers[k])
        solo = DeviceEnsembleSampler(counts[k], ndim, eng, mode=mode, rng='device', seed=seeds[k], chunk=3, moves=mix())
        solo.run_mcmc(p0s[k], n)
        group_same(dev, k, solo)
        kinds |= set(draws[k](0, n)[2].tolist())
    assert kinds == {0, 1}
    assert np.mean([a.mean() for a in dev.acceptance_fraction]) > 0.02
    # host-drawn: the targets' own NumPy generators, against GroupSampler with the same seeds
    hdev = DeviceGroupSampler(counts, ndim, grp, mode=mode, seeds=seeds, chunk=3, moves=mix())
    hdev.run_mcmc(p0s, n)
    htwin = GroupSampler(counts, ndim, fn, seeds=seeds, moves=mix())
    htwin.run_mcmc(p0s, n)
    for k in range(len(counts)):
        group_same(hdev, k, htwin.samplers[k])
    grp.close()


def test_each_member_of_a_group_walks_its_own_chain():
    """12 walkers: the smallest ensemble; 50: 25 active, odd; 514: 257 per half, one more than the step kernel's workgroup."""
    group_case('B', [12, 50, 514], [2**63 + 41, 42, 44], 6, 'logposterior', 1.0)


def test_triples_in_likelihood_mode():
    """ndim 8 (fac = 7 ln z on the stretch iterations, g0 = 2.38 / 4 on DE's), counts (16, 50)."""
    group_case('C', [16, 50], [300, 301], 8, 'loglikelihood', 0.1)


# ---- (e) the device series -------------------------------------------------------------------------------------------------
def test_the_device_series_holds_the_chains_rows():
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    from summary_numpy import flat_members
    eng, p0 = start(18)
    dev = DeviceEnsembleSampler(18, 6, eng, seed=SEED, chunk=CHUNK, rng='device', moves=mix(), autocorr='device')
    dev.run_mcmc(p0, 11)
    chain = dev.get_chain()
    assert np.array_equal(dev._series.read(0, 11), chain)
    got = dev.get_summary()
    flat = flat_members(chain, 11)[0]   # (tests/summary_numpy.py: the flat sample the summary is defined on)
    assert flat.shape == (11 * 18, 6) and got['count'] == len(flat)
    assert np.array_equal(got['min'], flat.min(axis=0)) and np.array_equal(got['max'], flat.max(axis=0))
    assert np.array_equal(got['quantiles'], np.quantile(flat, (0.16, 0.5, 0.84), axis=0).T)


# ---- (f) refusals through the ABI ----------------------------------------------------------------------------------------
def test_refusals_through_the_abi():
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.moves import DEMove, StretchMove, parse_moves
    eng, p0 = start(18)
    ctx = eng.ctx
    lp = eng.logposterior(p0)
    good = list(ctx.sampler_draw_moves(SEED, mix(), 0, 2, 18, 6))

    def refused(code, arrays=None, **kw):
        with pytest.raises(_lib.MsxError) as ei:
            if arrays is not None:
                ctx.sampler_enqueue_moves(0, *arrays)
            else:
                ctx.sampler_enqueue_moves_drawn(0, 2, SEED, **kw)
        assert ei.value.code == code, (ei.value, kw)

    ctx.sampler_policy(0)
    ctx.sampler_begin(_lib.MODE_LOGPOST, p0, lp, 2)
    bad = [a.copy() for a in good]
    bad[2][1] = 2                                  # an out-of-range kind
    refused(_lib.MSX_ERR_INVALID, bad)
    bad = [a.copy() for a in good]
    bad[2][:] = 1
    bad[4][0, 1, 3] = bad[3][0, 1, 3]              # p1 == p2 on a DE entry
    refused(_lib.MSX_ERR_INVALID, bad)
    bad = [a.copy() for a in good]
    bad[3][1, 0, 0] = 9                            # p1 past the complementary half
    refused(_lib.MSX_ERR_INVALID, bad)
    st = parse_moves(mix()).as_struct()
    st.weight[0] = 0.6                             # weights that do not sum to 1
    refused(_lib.MSX_ERR_INVALID, moves=st, first_iter=0)
    st = parse_moves(mix()).as_struct()
    st.kind[1] = 7
    refused(_lib.MSX_ERR_INVALID, moves=st, first_iter=0)
    refused(_lib.MSX_ERR_INVALID, moves=mix(), first_iter=-1)
    # nothing was queued: the run takes a host-fed chunk in the general layout, then a drawn one -- the all-drawn run
    ctx.sampler_enqueue_moves(0, *good)
    ctx.sampler_enqueue_moves_drawn(1, 2, SEED, mix(), 2)
    mixed = [ctx.sampler_collect(s, 2) for s in (0, 1)]
    assert ctx.sampler_overlapped() == 0
    ctx.sampler_end()
    ctx.sampler_begin(_lib.MODE_LOGPOST, p0, lp, 2)
    ctx.sampler_enqueue_moves_drawn(0, 2, SEED, mix(), 0)
    ctx.sampler_enqueue_moves_drawn(1, 2, SEED, mix(), 2)
    drawn = [ctx.sampler_collect(s, 2) for s in (0, 1)]
    ctx.sampler_end()
    for d, m in zip(drawn, mixed):
        assert np.array_equal(d[0], m[0]) and np.array_equal(d[1], m[1]) and np.array_equal(d[2], m[2]) and d[3] == m[3] == 0
    # a sharded run is stretch only
    ctx.sampler_begin(_lib.MODE_LOGPOST, p0, lp, 2)
    ctx.sampler_shard(0, 1)
    refused(_lib.MSX_ERR_STATE, moves=mix(), first_iter=0)
    refused(_lib.MSX_ERR_STATE, good)
    ctx.sampler_end()
    ctx.sampler_policy(-1)
    # the DE move needs two distinct walkers in each half
    with pytest.raises(_lib.MsxError) as ei:
        ctx.sampler_draw_moves(SEED, DEMove(), 0, 1, 2, 6)
    assert ei.value.code == _lib.MSX_ERR_INVALID
    assert ctx.sampler_draw_moves(SEED, StretchMove(), 0, 1, 2, 6)[2][0] == 0
