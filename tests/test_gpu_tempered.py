"""GPU: parallel tempering on the device-resident sampler (include/msx.h, msx_tempered_*; csrc/tempered_kernels.h; DESIGN.md
section 17).  The ladder runs BESIDE the fused kernel -- a step kernel proposes for all rungs, the plain evaluation scores the
proposals twice (prior, likelihood), the step kernel accepts, a swap kernel sweeps -- so (a) the device must walk the chain
of the host loop fed the device's own draws, (b) and of the host loop with the same seed when the host draws, (c) at the
shapes where the new kernels can go wrong, (d) those draws are the counter streams restated in NumPy, (e) a proposal outside
the prior is rejected whatever the likelihood reports there, and (f) the ABI refuses what it must."""
import numpy as np
import pytest

import common
from test_gpu_group_chain import spread
from test_gpu_overlap import _config2
from test_gpu_target_group import mixed_engines

pytestmark = pytest.mark.gpu

SEED = 17
CHUNK = 4     # runs of 5 then 6 iterations: chunks are crossed and end short
BETAS3 = [1.0, 0.5, 0.25]


def mix():
    from mcmc_spec_amd.moves import DEMove, StretchMove
    return [(StretchMove(), 0.5), (DEMove(), 0.4), (DEMove(gamma0=1.0), 0.1)]


def start(nw, T):
    """config 2's engine and a start (T, nw, 6) inside the prior: every rung its own walkers."""
    from mcmc_spec_amd import synth
    eng, W = _config2()
    p0 = synth.draw_walkers(nw * T, seed=5 + nw, tmin=W['tmin'], tmax=W['tmax']).reshape(T, nw, 6)
    return eng, p0


def two_runs(s, p0):
    """5 iterations, reset(), 6 more from where the first run ended."""
    st = s.run_mcmc(p0, 5)
    first = (s.get_chain(t=None).copy(), s.get_log_like(t=None).copy(), s.get_log_prior(t=None).copy(), s.acceptance_fraction.copy(),
             s.swap_fraction.copy(), st)
    s.reset()
    s.run_mcmc(st, 6)
    return first


def same_state(a, b):
    assert np.array_equal(a.coords, b.coords) and np.array_equal(a.log_like, b.log_like) and np.array_equal(a.log_prior, b.log_prior)


def same_run(a, fa, b, fb, n=6):
    for x, y in zip(fa[:5], fb[:5]):
        assert np.array_equal(x, y)
    same_state(fa[5], fb[5])
    assert a.get_chain(t=None).shape[0] == n
    assert np.array_equal(a.get_chain(t=None), b.get_chain(t=None))
    assert np.array_equal(a.get_log_like(t=None), b.get_log_like(t=None)) and np.array_equal(a.get_log_prior(t=None), b.get_log_prior(t=None))
    assert np.array_equal(a.get_log_prob(0), b.get_log_prob(0))
    assert np.array_equal(a.acceptance_fraction, b.acceptance_fraction) and np.array_equal(a.swap_fraction, b.swap_fraction)
    same_state(a.get_last_sample(), b.get_last_sample())


def twin_of(eng, nw, ndim, betas, seeds, moves):
    from mcmc_spec_amd.tempered import TemperedSampler
    return TemperedSampler(nw, ndim, eng, betas=betas, seeds=seeds, moves=moves,
                           draws=lambda i, m: eng.ctx.tempered_draw(seeds, moves, i, m, nw, ndim))


# ---- (a) device-drawn: the device walks the host twin's chain ----------------------------------------------------------------
@pytest.mark.parametrize('nw', [18, 256])
def test_the_ladder_walks_the_host_twins_chain(nw):
    """18 walkers: 9 per half, a fraction of a wave; 256: 768 walkers in the run."""
    from mcmc_spec_amd.tempered import DeviceTemperedSampler
    eng, p0 = start(nw, 3)
    dev = DeviceTemperedSampler(nw, 6, eng, betas=BETAS3, seed=SEED, chunk=CHUNK, rng='device', moves=mix())
    assert dev.seeds == [SEED, SEED + 1, SEED + 2]
    fd = two_runs(dev, p0)
    host = twin_of(eng, nw, 6, BETAS3, dev.seeds, mix())
    fh = two_runs(host, p0)
    same_run(dev, fd, host, fh)
    assert dev._drawn == 11 == host._drawn
    swaps = fd[4] * 5 * nw + dev.swap_fraction * 6 * nw
    print('swaps per pair over the 11 iterations:', swaps, 'of', 11 * nw, ' acceptance', dev.acceptance_fraction.mean(axis=1))
    assert np.all(swaps > 0) and np.all(swaps < 11 * nw)             # accepted and refused swaps both occur
    assert 0.02 < dev.acceptance_fraction.mean() < 0.95
    fresh = DeviceTemperedSampler(nw, 6, eng, betas=BETAS3, seed=SEED, chunk=CHUNK, rng='device', moves=mix())   # (would replay 0..5)
    fresh.run_mcmc(fd[5], 6)
    assert not np.array_equal(fresh.get_chain(t=None), dev.get_chain(t=None))


# ---- (b) host-drawn ----------------------------------------------------------------------------------------------------------------
def test_the_host_drawn_ladder_walks_the_host_loops_chain():
    from mcmc_spec_amd.tempered import DeviceTemperedSampler, TemperedSampler
    eng, p0 = start(18, 3)
    dev = DeviceTemperedSampler(18, 6, eng, betas=BETAS3, seed=SEED, chunk=CHUNK, moves=mix())
    fd = two_runs(dev, p0)
    host = TemperedSampler(18, 6, eng, betas=BETAS3, seed=SEED, moves=mix())
    fh = two_runs(host, p0)
    same_run(dev, fd, host, fh)


# ---- (c) shapes ------------------------------------------------------------------------------------------------------------------------
def one_run(eng, p0, betas, moves, n, chunk=CHUNK):
    from mcmc_spec_amd.tempered import DeviceTemperedSampler
    T, nw, ndim = p0.shape
    dev = DeviceTemperedSampler(nw, ndim, eng, betas=betas, seed=SEED, chunk=chunk, rng='device', moves=moves)
    dev.run_mcmc(p0, n)
    host = twin_of(eng, nw, ndim, betas, dev.seeds, moves)
    host.run_mcmc(p0, n)
    assert np.array_equal(dev.get_chain(t=None), host.get_chain(t=None))
    assert np.array_equal(dev.get_log_like(t=None), host.get_log_like(t=None)) and np.array_equal(dev.get_log_prior(t=None), host.get_log_prior(t=None))
    assert np.array_equal(dev.acceptance_fraction, host.acceptance_fraction) and np.array_equal(dev.swap_fraction, host.swap_fraction)
    return dev, host


def test_one_more_walker_than_the_step_kernels_workgroup():
    """T = 2, 514 walkers: 257 per half; the swap kernel takes three workgroups, the last one nearly empty."""
    eng, p0 = start(514, 2)
    dev, _ = one_run(eng, p0, [1.0, 0.3], mix(), 5)
    assert np.all(dev.swap_fraction > 0) and np.all(dev.swap_fraction < 1)


def test_a_launch_of_2048_proposals_takes_the_pair_form():
    """T = 8, 512 walkers, 3 iterations: 2,048 proposals per launch.  The twin evaluates through the same engine; the forms
    give the same bits."""
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.moves import StretchMove
    from mcmc_spec_amd.tempered import DeviceTemperedSampler, default_betas
    eng, p0 = start(512, 8)
    betas = default_betas(8, 0.02)
    dev = DeviceTemperedSampler(512, 6, eng, betas=betas, seed=SEED, chunk=CHUNK, rng='device')
    dev.run_mcmc(p0, 3)
    assert eng.ctx.last_form() == _lib.FORM_PAIR
    host = twin_of(eng, 512, 6, betas, dev.seeds, StretchMove())
    host.run_mcmc(p0, 3)
    assert np.array_equal(dev.get_chain(t=None), host.get_chain(t=None)) and np.array_equal(dev.get_log_like(t=None), host.get_log_like(t=None))
    assert np.array_equal(dev.swap_fraction, host.swap_fraction) and np.array_equal(dev.acceptance_fraction, host.acceptance_fraction)


def test_triples():
    """T = 2, 16 walkers, ndim 8 (fac = 7 ln z on the stretch iterations, g0 = 2.38 / 4 on DE's)."""
    from mcmc_spec_amd import _lib
    c, engines = mixed_engines('C')
    eng = engines[0]
    cand = spread(c, 400, 500, 0.1)
    cand[:, 1:c.nspec] += 100.0
    lpr, st = eng.ctx.logprob_batch(cand, _lib.MODE_LOGPRIOR)
    ll, stl = eng.ctx.logprob_batch(cand, _lib.MODE_LOGLIKE)
    ok = np.isfinite(lpr) & (st == 0) & (stl == 0)
    assert ok.sum() >= 32, ok.sum()
    p0 = cand[ok][:32].reshape(2, 16, 8)
    dev, _ = one_run(eng, p0, [1.0, 0.4], mix(), 7, chunk=3)
    assert dev.acceptance_fraction.mean() > 0.02


def test_one_rung_against_the_twin():
    eng, p0 = start(18, 1)
    dev, host = one_run(eng, p0, [1.0], mix(), 6)
    assert dev.swap_fraction.shape == (0,) and dev.get_chain().shape == (6, 18, 6)


# ---- (d) the draw --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nw,T', [(18, 3), (256, 8)])
def test_the_device_draws_are_the_counter_streams_restated_in_numpy(nw, T):
    from mcmc_spec_amd.tempered import counter_swap_logu
    eng, W = _config2()
    seeds = [2**63 + 5 + 7 * t for t in range(T)]
    members, swap_logu = eng.ctx.tempered_draw(seeds, mix(), 0, 11, nw, 6)
    assert len(members) == T and swap_logu.shape == (11, T - 1, nw)
    for t in range(T):
        solo = eng.ctx.sampler_draw_moves(seeds[t], mix(), 0, 11, nw, 6)
        for i in range(8):   # the member's arrays are msx_sampler_draw_moves' for seeds[t]: integers and doubles alike
            assert members[t][i].dtype == solo[i].dtype and np.array_equal(members[t][i], solo[i]), (t, i)
    want = counter_swap_logu(seeds[0], 0, 11, T, nw)
    assert np.allclose(swap_logu, want, rtol=4e-16, atol=1e-300)
    assert np.all(swap_logu <= 0.0) and len(np.unique(swap_logu)) == swap_logu.size
    later_m, later_s = eng.ctx.tempered_draw(seeds, mix(), 4, 7, nw, 6)   # a later chunk is the stream's later rows
    assert np.array_equal(later_s, swap_logu[4:])
    assert all(np.array_equal(a, b[4:]) for t in range(T) for a, b in zip(later_m[t], members[t]))


# ---- (e) statuses --------------------------------------------------------------------------------------------------------------------
def test_a_proposal_outside_the_prior_is_rejected_whatever_the_likelihood_reports():
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.moves import StretchMove
    from mcmc_spec_amd.tempered import TemperedSampler
    nw, T, hot = 18, 3, 2
    eng, p0 = start(nw, T)
    ctx = eng.ctx
    seeds = [SEED, SEED + 1, SEED + 2]
    members, swap_logu = ctx.tempered_draw(seeds, StretchMove(), 0, 1, nw, 6)
    sidx, cidx, kind, p1, p2, g, fac, logu = (np.stack([m[i] for m in members], axis=1) for i in range(8))
    # one stretch entry of the hot rung's first half-step whose factor carries the walker's Teff beyond the grid and the
    # prior box, and where the likelihood ALONE reports an error status (otherwise this test shows nothing)
    found = None
    for j in range(nw // 2):
        s = p0[hot, sidx[0, hot, 0, j]]
        c = p0[hot, cidx[0, hot, 0, p1[0, hot, 0, j]]]
        for z in (20.0, 50.0, 100.0, 200.0, 500.0):
            q = (c - (c - s) * z)[None]
            (_, st_p), (_, st_l) = ctx.logprob_batch(q, _lib.MODE_LOGPRIOR), ctx.logprob_batch(q, _lib.MODE_LOGLIKE)
            if st_p[0] == _lib.W_REJECT and st_l[0] > _lib.W_REJECT:
                found = (j, z, int(st_l[0]))
                break
        if found:
            break
    assert found is not None
    j, z, code = found
    print('entry', j, 'factor', z, 'likelihood status', code)
    g[0, hot, 0, j], fac[0, hot, 0, j], logu[0, hot, 0, j] = z, 5.0 * np.log(z), -1e300   # (any finite density would be accepted)
    swap_logu[:] = 1e300                                                                  # no swaps: the walker is found where it was
    lpr, ll = ctx.logprob_batch(p0.reshape(-1, 6), _lib.MODE_LOGPRIOR)[0].reshape(T, nw), ctx.logprob_batch(p0.reshape(-1, 6), _lib.MODE_LOGLIKE)[0].reshape(T, nw)
    ctx.sampler_policy(0)
    ctx.tempered_begin(BETAS3, p0, ll, lpr, 2)
    try:
        ctx.tempered_enqueue(0, sidx, cidx, kind, p1, p2, g, fac, logu, swap_logu)
        chain, llc, lprc, nacc, nswap, worst = ctx.tempered_collect(0, 1)
    finally:
        ctx.tempered_end()
        ctx.sampler_policy(-1)
    w = sidx[0, hot, 0, j]
    assert worst.tolist() == [0, 0, 0] and nswap.tolist() == [0, 0]
    assert np.array_equal(chain[0, hot, w], p0[hot, w]) and nacc[hot, w] == 0 and llc[0, hot, w] == ll[hot, w]
    assert nacc.sum() > 0
    # the host loop under the same draws: the same rule, the same chain
    arrays = [tuple(a[:, t] for a in (sidx, cidx, kind, p1, p2, g, fac, logu)) for t in range(T)]
    host = TemperedSampler(nw, 6, eng, betas=BETAS3, seeds=seeds, draws=lambda i, m: (arrays, swap_logu))
    host.run_mcmc(p0, 1)
    assert np.array_equal(host.get_chain(t=None)[0], chain[0]) and np.array_equal(host.get_log_like(t=None)[0], llc[0])
    assert np.array_equal(host.get_log_prior(t=None)[0], lprc[0]) and np.array_equal(host.acceptance_fraction, nacc)


# ---- (f) refusals through the ABI ------------------------------------------------------------------------------------------------
def test_refusals_through_the_abi():
    from common import golden_case
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.moves import DEMove, parse_moves
    from test_gpu_parity import make_engine
    nw, T = 18, 3
    eng, p0 = start(nw, T)
    ctx = eng.ctx
    flat = p0.reshape(-1, 6)
    lpr, ll = ctx.logprob_batch(flat, _lib.MODE_LOGPRIOR)[0].reshape(T, nw), ctx.logprob_batch(flat, _lib.MODE_LOGLIKE)[0].reshape(T, nw)
    seeds = [SEED, SEED + 1, SEED + 2]

    def raises(code, fn, *a, **kw):
        with pytest.raises(_lib.MsxError) as ei:
            fn(*a, **kw)
        assert ei.value.code == code, ei.value

    def begin(betas=BETAS3, coords=p0, ll=ll, lpr=lpr, c=ctx):
        betas = np.asarray(betas, dtype=float)
        n = len(betas)
        c.tempered_begin(betas, coords[:1].repeat(n, 0) if n != len(coords) else coords, ll[:1].repeat(n, 0) if n != len(ll) else ll,
                         lpr[:1].repeat(n, 0) if n != len(lpr) else lpr, 2)

    # ---- begin: MSX_ERR_STATE ----
    ctx.sampler_policy(-1)
    raises(_lib.MSX_ERR_STATE, begin)                                         # an overlapped policy
    ctx.sampler_policy(0)
    bare = _lib.Context(0)
    bare.sampler_policy(0)
    raises(_lib.MSX_ERR_STATE, begin, c=bare)                                 # no problem staged
    bare.close()
    ctx.sampler_begin(_lib.MODE_LOGPOST, p0[0], lpr[0] + ll[0], 2)
    raises(_lib.MSX_ERR_STATE, begin)                                         # a sampler run in flight
    ctx.sampler_end()
    c = golden_case('B')
    ranks = [make_engine(c, rad_prior=False) for _ in range(2)]
    _lib.Context.comm_init_loopback([e.ctx for e in ranks])
    q0 = np.repeat(spread(c, nw, 3)[None], T, axis=0)
    ranks[0].ctx.sampler_policy(0)
    raises(_lib.MSX_ERR_STATE, ranks[0].ctx.tempered_begin, np.array(BETAS3), q0, np.zeros((T, nw)), np.zeros((T, nw)), 2)   # a communicator
    # ---- begin: MSX_ERR_INVALID ----
    for betas in ([1.0, 0.5, 0.5], [0.5, 1.0, 2.0], [1.0, 0.5, 0.0], [1.0, 0.5, -0.1], [1.0, float('nan'), 0.1], [float('inf'), 1.0, 0.5],
                  np.geomspace(1.0, 0.01, 65)):
        raises(_lib.MSX_ERR_INVALID, begin, betas=betas)
    raises(_lib.MSX_ERR_INVALID, ctx.tempered_begin, np.array(BETAS3), p0[:, :17], ll[:, :17], lpr[:, :17], 2)       # odd
    raises(_lib.MSX_ERR_INVALID, ctx.tempered_begin, np.array(BETAS3), p0[:, :1], ll[:, :1], lpr[:, :1], 2)          # < 2
    raises(_lib.MSX_ERR_INVALID, lambda: ctx.check(ctx.lib.msx_tempered_begin(
        ctx.h, 0, _lib.dptr(np.array(BETAS3)), nw, 6, 2, _lib.dptr(p0), _lib.dptr(ll), _lib.dptr(lpr))))             # no rungs
    bad = lpr.copy()
    bad[1, 4] = -np.inf
    raises(_lib.MSX_ERR_INVALID, begin, lpr=bad)                              # an initial walker outside the prior box
    bad = ll.copy()
    bad[2, 0] = np.nan
    raises(_lib.MSX_ERR_INVALID, begin, ll=bad)
    # ---- a run: refused chunks queue nothing ----
    begin()
    raises(_lib.MSX_ERR_STATE, begin)                                         # a tempered run in flight
    raises(_lib.MSX_ERR_STATE, ctx.sampler_begin, _lib.MODE_LOGPOST, p0[0], lpr[0] + ll[0], 2)
    series = _lib.Series(ctx, nw, 6)
    raises(_lib.MSX_ERR_STATE, ctx.sampler_attach_series, series, 0)
    members, swap_logu = ctx.tempered_draw(seeds, mix(), 0, 2, nw, 6)
    good = [np.stack([m[i] for m in members], axis=1) for i in range(8)] + [swap_logu]

    def fed(code, arrays):
        raises(code, ctx.tempered_enqueue, 0, *arrays)

    def drawn(code, **kw):
        args = dict(seeds=seeds, moves=mix(), first_iter=0)
        args.update(kw)
        raises(code, ctx.tempered_enqueue_drawn, 0, 2, args['seeds'], args['moves'], args['first_iter'])

    bad = [a.copy() for a in good]
    bad[2][1, 2] = 2                                   # an out-of-range kind
    fed(_lib.MSX_ERR_INVALID, bad)
    bad = [a.copy() for a in good]
    bad[2][:] = 1
    bad[4][0, 1, 1, 3] = bad[3][0, 1, 1, 3]            # p1 == p2 on a DE entry
    fed(_lib.MSX_ERR_INVALID, bad)
    bad = [a.copy() for a in good]
    bad[3][1, 2, 0, 0] = 9                             # p1 past the complementary half
    fed(_lib.MSX_ERR_INVALID, bad)
    bad = [a.copy() for a in good]
    bad[0][0, 0, 1, 2] = nw                            # a walker index past the rung
    fed(_lib.MSX_ERR_INVALID, bad)
    st = parse_moves(mix()).as_struct()
    st.weight[0] = 0.6                                 # weights that do not sum to 1
    drawn(_lib.MSX_ERR_INVALID, moves=st)
    drawn(_lib.MSX_ERR_INVALID, first_iter=-1)
    raises(_lib.MSX_ERR_INVALID, ctx.tempered_enqueue_drawn, 0, 3, seeds, mix(), 0)      # longer than the run's chunks
    raises(_lib.MSX_ERR_INVALID, ctx.tempered_enqueue_drawn, 2, 2, seeds, mix(), 0)      # no such slot
    raises(_lib.MSX_ERR_STATE, ctx.tempered_collect, 0, 2)                               # nothing was queued
    # the run takes a host-fed chunk, then a drawn one: the all-drawn run
    ctx.tempered_enqueue(0, *good)
    raises(_lib.MSX_ERR_STATE, ctx.tempered_enqueue_drawn, 0, 2, seeds, mix(), 2)        # slot not collected yet
    ctx.tempered_enqueue_drawn(1, 2, seeds, mix(), 2)
    mixed = [ctx.tempered_collect(s, 2) for s in (0, 1)]
    end_mixed = ctx.tempered_end(want_state=True)
    begin()
    ctx.tempered_enqueue_drawn(0, 2, seeds, mix(), 0)
    ctx.tempered_enqueue_drawn(1, 2, seeds, mix(), 2)
    alldrawn = [ctx.tempered_collect(s, 2) for s in (0, 1)]
    end_drawn = ctx.tempered_end(want_state=True)
    for d, m in zip(alldrawn, mixed):
        assert all(np.array_equal(x, y) for x, y in zip(d, m)) and d[5].tolist() == [0, 0, 0]
    assert all(np.array_equal(x, y) for x, y in zip(end_drawn, end_mixed)) and np.array_equal(end_drawn[0], alldrawn[1][0][-1])
    assert ctx.tempered_end() is None                                                    # no run: nothing to end
    raises(_lib.MSX_ERR_STATE, ctx.tempered_collect, 0, 2)
    raises(_lib.MSX_ERR_STATE, ctx.tempered_enqueue_drawn, 0, 2, seeds, mix(), 0)
    # the DE move needs two distinct walkers in each half; the device generator takes up to 4096 walkers
    raises(_lib.MSX_ERR_INVALID, ctx.tempered_draw, seeds, DEMove(), 0, 1, 2, 6)
    raises(_lib.MSX_ERR_INVALID, ctx.tempered_draw, seeds, mix(), 0, 1, 4098, 6)
    # the context is as it was: the default sampler runs
    ctx.sampler_policy(-1)
    ctx.sampler_begin(_lib.MODE_LOGPOST, p0[0], lpr[0] + ll[0], 2)
    ctx.sampler_end()
