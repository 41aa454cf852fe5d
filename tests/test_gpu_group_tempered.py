"""GPU: parallel tempering for a target group (include/msx.h, msx_group_tempered_* / msx_group_ladder_*;
csrc/group_tempered_kernels.h; mcmc_spec_amd.tempered.DeviceGroupTemperedSampler).  K targets x T rungs
share every launch, so the pin throughout is that TARGET k OF THE GROUP RUN EQUALS ``DeviceTemperedSampler`` ON ENGINE k ALONE
WITH ``seeds[k]`` -- chain, ll, lpr, acceptance and swap fractions, last state, bit for bit, across 5 iterations, reset(), 6
more in chunks of 4 -- at the shapes where the new kernels can go wrong; then the adaptive ladders, the device series, the
prior-reject rule, the error that names its target, and what the ABI refuses."""
import numpy as np
import pytest

import common
from test_gpu_adaptive import gathered, ladders, same_ladders
from test_gpu_group_chain import spread
from test_gpu_overlap import _config2
from test_gpu_target_group import _stage, koi_engines, mixed_engines
from test_gpu_tempered import CHUNK, mix, same_run, two_runs

pytestmark = pytest.mark.gpu


def inside(eng, c, n, seed, scale=0.3, shift=0.0):
    """n walkers around golden case c's theta (primary moved by ``shift`` K) that ``eng`` places inside its prior with a clean
    likelihood."""
    from mcmc_spec_amd import _lib
    cand = spread(c, 3 * n + 64, seed, scale)
    cand[:, 0] += shift
    cand[:, 1:c.nspec] += 100.0
    lpr, st = eng.ctx.logprob_batch(cand, _lib.MODE_LOGPRIOR)
    ll, stl = eng.ctx.logprob_batch(cand, _lib.MODE_LOGLIKE)
    ok = np.isfinite(lpr) & (st == 0) & (stl == 0) & np.isfinite(ll)
    assert ok.sum() >= n, (ok.sum(), n)
    return cand[ok][:n]


def group_of(grp, counts, ndim, betas, seeds, rng='device', moves=mix, **kw):
    from mcmc_spec_amd.tempered import DeviceGroupTemperedSampler
    return DeviceGroupTemperedSampler(grp, counts, ndim, betas=betas, seeds=seeds, chunk=CHUNK, rng=rng, moves=moves(), **kw)


def solo_of(eng, nw, ndim, betas, seed, rng='device', moves=mix, **kw):
    from mcmc_spec_amd.tempered import DeviceTemperedSampler
    seed, seeds = (seed, None) if np.ndim(seed) == 0 else (None, seed)
    return DeviceTemperedSampler(nw, ndim, eng, betas=betas, seed=seed, seeds=seeds, chunk=CHUNK, rng=rng, moves=moves(), **kw)


def snapshot(v, st):
    return (v.get_chain(t=None).copy(), v.get_log_like(t=None).copy(), v.get_log_prior(t=None).copy(), v.acceptance_fraction.copy(),
            v.swap_fraction.copy(), st)


def two_group_runs(s, p0s, **kw):
    """test_gpu_tempered.two_runs for every target at once; also the ladders after the first run."""
    st = s.run_mcmc(p0s, 5, **kw)
    first = [snapshot(s.target(k), st[k]) for k in range(len(p0s))]
    lad = [ladders(s.target(k)) for k in range(len(p0s))]
    s.reset()
    s.run_mcmc(st, 6, **kw)
    return first, lad


def pinned_to_the_solo_runs(s, first, engines, counts, ndim, betas, seeds, p0s, **kw):
    """Every target of the finished two_group_runs against its own DeviceTemperedSampler; the solo samplers."""
    out = []
    for k, eng in enumerate(engines):
        one = solo_of(eng, counts[k], ndim, betas[k], seeds[k], **kw)
        f1 = two_runs(one, p0s[k])
        same_run(s.target(k), first[k], one, f1)
        assert s.target(k)._drawn == one._drawn == (11 if kw.get('rng', 'device') == 'device' else 0)
        out.append(one)
    return out


# ---- 1. mixed members, unequal counts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rng', ['device', 'host'])
def test_mixed_members_with_unequal_counts_walk_their_own_ladders(rng):
    """Three members that differ (as staged, cropped, dist_fit off), T = 3, counts (18, 34, 20): 9 per half is a fraction of a
    wave; the section-16 mixture; a ladder of its own per target."""
    from mcmc_spec_amd.group import TargetGroup
    c, engines = mixed_engines('B')
    members, counts, T = engines[:3], [18, 34, 20], 3
    betas = [[1.0, 0.5, 0.25], [1.0, 0.4, 0.1], [1.0, 0.7, 0.3]]
    seeds = [17, 2**63 + 4, [5, 99, 12345]]
    p0s = [inside(e, c, T * n, 40 + k).reshape(T, n, 6) for k, (e, n) in enumerate(zip(members, counts))]
    grp = TargetGroup(members)
    s = group_of(grp, counts, 6, betas, seeds, rng=rng)
    first, _ = two_group_runs(s, p0s)
    pinned_to_the_solo_runs(s, first, members, counts, 6, betas, seeds, p0s, rng=rng)
    assert not np.array_equal(s.target(0).get_chain(t=None), s.target(1).get_chain(t=None)[:, :, :18])
    for k in range(3):
        swaps = first[k][4] * 5 * counts[k] + s.target(k).swap_fraction * 6 * counts[k]
        print('target', k, 'swaps per pair over the 11 iterations:', swaps, 'of', 11 * counts[k], ' acceptance',
              s.target(k).acceptance_fraction.mean(axis=1))
        assert np.all(swaps > 0) and np.all(swaps < 11 * counts[k])          # accepted and refused swaps both occur
        assert 0.02 < s.target(k).acceptance_fraction.mean() < 0.95
    if rng == 'device':   # ... and so equals its host twin
        from mcmc_spec_amd.tempered import TemperedSampler
        k, eng = 1, members[1]
        sd = s.target(k).seeds
        host = TemperedSampler(counts[k], 6, eng, betas=betas[k], seeds=sd, moves=mix(),
                               draws=lambda i, m: eng.ctx.tempered_draw(sd, mix(), i, m, counts[k], 6))
        same_run(s.target(k), first[k], host, two_runs(host, p0s[k]))
    grp.close()


# ---- 2. one more walker than a workgroup ---------------------------------------------------------------------------------------
def test_one_more_walker_than_the_step_kernels_workgroup():
    """Counts (514, 18), T = 2: 257 per half is one more than the step kernel's workgroup; the sweep has three workgroups for
    target 0 and two idle ones for target 1."""
    from mcmc_spec_amd.group import TargetGroup
    c, engines = mixed_engines('B')
    members, counts, T = engines[:2], [514, 18], 2
    betas, seeds = [[1.0, 0.3]] * 2, [3, 4]
    p0s = [inside(e, c, T * n, 50 + k).reshape(T, n, 6) for k, (e, n) in enumerate(zip(members, counts))]
    grp = TargetGroup(members)
    s = group_of(grp, counts, 6, betas[0], seeds)       # (one ladder for all targets)
    first, _ = two_group_runs(s, p0s)
    pinned_to_the_solo_runs(s, first, members, counts, 6, betas, seeds, p0s)
    assert all(np.all(s.target(k).swap_fraction > 0) and np.all(s.target(k).swap_fraction < 1) for k in range(2))
    grp.close()


# ---- 3. the member table full ------------------------------------------------------------------------------------------------------
def test_the_member_table_full():
    """8 KOI targets x 8 rungs x 8 walkers, 3 iterations: K T = 64 (through the ABI: the Python samplers ask for 2 ndim
    walkers).  A 9th rung or a 9th target is refused."""
    from mcmc_spec_amd import _lib, synth
    from mcmc_spec_amd.group import TargetGroup
    from mcmc_spec_amd.moves import StretchMove
    from mcmc_spec_amd.tempered import default_betas
    g, tags, engines = koi_engines()
    c = common.golden_case('A')
    K, T, nw = 8, 8, 8
    betas = default_betas(T, 0.05)
    seeds = [[100 + 10 * k + t for t in range(T)] for k in range(K)]
    p0s, lprs, lls = [], [], []
    for k in range(K):   # starts inside the prior with a clean likelihood
        cand = synth.draw_walkers(4 * T * nw, seed=70 + k, tmin=c.tmin, tmax=c.tmax)
        (lpr, st), (ll, stl) = engines[k].ctx.logprob_batch(cand, _lib.MODE_LOGPRIOR), engines[k].ctx.logprob_batch(cand, _lib.MODE_LOGLIKE)
        ok = np.isfinite(lpr) & (st == 0) & (stl == 0) & np.isfinite(ll)
        assert ok.sum() >= T * nw, (k, ok.sum())
        p0s.append(cand[ok][:T * nw]), lprs.append(lpr[ok][:T * nw]), lls.append(ll[ok][:T * nw])
    grp = TargetGroup(engines[:K])
    grp.group.tempered_begin(np.tile(betas, (K, 1)), [nw] * K, np.concatenate(p0s), np.concatenate(lls), np.concatenate(lprs), 4)
    grp.group.tempered_enqueue_drawn(0, 3, seeds, StretchMove(), 0)
    got = grp.group.tempered_collect(0, 3)
    end = grp.group.tempered_end(want_state=True)
    assert got[5].shape == (K, T) and not got[5].any() and got[4].shape == (K, T - 1)
    for k in range(K):
        ctx = engines[k].ctx
        ctx.sampler_policy(0)
        try:
            ctx.tempered_begin(betas, p0s[k].reshape(T, nw, 6), lls[k].reshape(T, nw), lprs[k].reshape(T, nw), 4)
            ctx.tempered_enqueue_drawn(0, 3, seeds[k], StretchMove(), 0)
            chain, llc, lprc, nacc, nswap, worst = ctx.tempered_collect(0, 3)
            one_end = ctx.tempered_end(want_state=True)
        finally:
            ctx.tempered_end()
            ctx.sampler_policy(-1)
        sl = slice(k * T * nw, (k + 1) * T * nw)
        assert np.array_equal(got[0][:, sl].reshape(3, T, nw, 6), chain) and np.array_equal(got[1][:, sl].reshape(3, T, nw), llc)
        assert np.array_equal(got[2][:, sl].reshape(3, T, nw), lprc) and np.array_equal(got[3][sl].reshape(T, nw), nacc)
        assert np.array_equal(got[4][k], nswap) and not worst.any()
        assert np.array_equal(end[0][sl].reshape(T, nw, 6), one_end[0]) and np.array_equal(end[1][sl].reshape(T, nw), one_end[1])
    assert got[3].sum() > 0 and got[4].sum() > 0 and not np.array_equal(got[0][:, :T * nw], got[0][:, T * nw:2 * T * nw])

    def refused(group, k, ntemps):
        W = k * ntemps * nw
        with pytest.raises(_lib.MsxError) as ei:
            group.group.tempered_begin(np.tile(default_betas(ntemps, 0.05), (k, 1)), [nw] * k, np.zeros((W, 6)), np.zeros(W), np.zeros(W), 2)
        assert ei.value.code == _lib.MSX_ERR_INVALID, ei.value
    refused(grp, 8, 9)
    nine = TargetGroup(engines[:9])
    refused(nine, 9, 8)
    nine.close()
    grp.close()


# ---- 4. a group of one ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('adaptive', [False, True])
def test_a_group_of_one_is_the_single_ladder(adaptive):
    from mcmc_spec_amd import synth
    from mcmc_spec_amd.group import TargetGroup
    from mcmc_spec_amd.tempered import default_betas
    eng, W = _config2()
    nw, T = 18, 3
    p0 = synth.draw_walkers(nw * T, seed=5 + nw, tmin=W['tmin'], tmax=W['tmax']).reshape(T, nw, 6)
    kw = dict(adaptive=True, adaptation_lag=8.0, adaptation_time=2.0) if adaptive else {}
    if adaptive:
        p0 = gathered(p0)
    betas = default_betas(T, 0.02)
    grp = TargetGroup([eng])
    s = group_of(grp, [nw], 6, betas, [17], **kw)
    first, lad = two_group_runs(s, [p0])
    one = solo_of(eng, nw, 6, betas, 17, **kw)
    f1 = two_runs(one, p0)
    same_run(s.target(0), first[0], one, f1)
    same_ladders(ladders(s.target(0)), ladders(one))
    if adaptive:
        assert not np.array_equal(s.target(0).betas, betas) and s.target(0)._adapted == 11 and lad[0][3] == 5
    else:
        assert np.all(s.target(0).get_betas() == betas) and s.target(0)._adapted == 0
    grp.close()


# ---- 5. triples ------------------------------------------------------------------------------------------------------------------------
def test_triples():
    """nspec = 3: ndim 8 (fac = 7 ln z on the stretch iterations, g0 = 2.38 / 4 on DE's); T = 2, counts (16, 20)."""
    from mcmc_spec_amd.group import TargetGroup
    c, engines = mixed_engines('C')
    members, counts, T = engines[:2], [16, 20], 2
    betas, seeds = [[1.0, 0.4], [1.0, 0.6]], [8, 9]
    p0s = [inside(e, c, T * n, 500 + k, scale=0.1).reshape(T, n, 8) for k, (e, n) in enumerate(zip(members, counts))]
    grp = TargetGroup(members)
    s = group_of(grp, counts, 8, betas, seeds)
    first, _ = two_group_runs(s, p0s)
    pinned_to_the_solo_runs(s, first, members, counts, 8, betas, seeds, p0s)
    assert s.target(0).acceptance_fraction.mean() > 0.02
    grp.close()


# ---- 6. adaptive ---------------------------------------------------------------------------------------------------------------------
def test_every_target_adapts_its_own_ladder():
    """K = 2, T = 4, lag 10, time 1: the ladders move within 11 iterations, each as its solo adaptive run's."""
    from mcmc_spec_amd.group import TargetGroup
    from mcmc_spec_amd.tempered import default_betas
    c, engines = mixed_engines('B')
    members, counts, T = engines[:2], [18, 26], 4
    betas, seeds = [default_betas(T, 0.02), default_betas(T, 0.05)], [31, 32]
    kw = dict(adaptive=True, adaptation_lag=10.0, adaptation_time=1.0)
    p0s = [gathered(inside(e, c, T * n, 60 + k).reshape(T, n, 6)) for k, (e, n) in enumerate(zip(members, counts))]
    grp = TargetGroup(members)
    s = group_of(grp, counts, 6, betas, seeds, **kw)
    first, lad = two_group_runs(s, p0s)
    ones = []
    for k, eng in enumerate(members):
        one = solo_of(eng, counts[k], 6, betas[k], seeds[k], **kw)
        st = one.run_mcmc(p0s[k], 5)
        f1, l1 = snapshot(one, st), ladders(one)
        one.reset()
        one.run_mcmc(st, 6)
        same_run(s.target(k), first[k], one, f1)
        same_ladders(lad[k], l1)
        same_ladders(ladders(s.target(k)), ladders(one))
        assert s.target(k).get_betas().tobytes() == one.get_betas().tobytes() and s.target(k)._adapted == 11
        assert not np.array_equal(s.target(k).betas[1:-1], betas[k][1:-1])                  # the ladder moved
        assert s.target(k).betas[0] == 1.0 and s.target(k).betas[-1] == betas[k][-1]
        ones.append(one)
    print('ladders after 11 iterations:', s.target(0).betas, s.target(1).betas)
    assert not np.array_equal(s.target(0).betas, s.target(1).betas)                          # the two targets' ladders end different
    # adapt=False on the next run freezes them
    frozen = [s.target(k).betas.copy() for k in range(2)]
    st = s.run_mcmc([s.target(k).get_last_sample() for k in range(2)], 5, adapt=False)
    for k in range(2):
        ones[k].run_mcmc(ones[k].get_last_sample(), 5, adapt=False)
        assert np.array_equal(s.target(k).get_chain(t=None), ones[k].get_chain(t=None))
        assert np.all(s.target(k).get_betas()[6:] == frozen[k]) and np.array_equal(s.target(k).betas, frozen[k]) and s.target(k)._adapted == 11
        with pytest.raises(ValueError, match='adapt=False'):                               # the moving rows are refused
            s.target(k).log_evidence(blocks=2)
        assert np.isfinite(s.target(k).log_evidence(discard=6, blocks=2).log_z)
    grp.close()


# ---- 7. the device series ----------------------------------------------------------------------------------------------------------
def test_the_device_series_serve_every_target():
    """autocorr='device': ONE pair of series of K T members; target(k)'s summary, autocorrelation time and evidence are the solo
    device run's values exactly, and the chain is the same bits whatever autocorr is."""
    from mcmc_spec_amd.group import TargetGroup
    c, engines = mixed_engines('B')
    members, counts, T = engines[:2], [18, 12], 3
    betas, seeds = [[1.0, 0.5, 0.25], [1.0, 0.4, 0.1]], [21, 22]
    p0s = [inside(e, c, T * n, 80 + k).reshape(T, n, 6) for k, (e, n) in enumerate(zip(members, counts))]
    grp = TargetGroup(members)
    s = group_of(grp, counts, 6, betas, seeds, autocorr='device')
    first, _ = two_group_runs(s, p0s)
    plain = group_of(grp, counts, 6, betas, seeds)
    fp, _ = two_group_runs(plain, p0s)
    assert s._series.k == 2 * T and s._series.rows == 6 == s._dens.rows
    rows = np.concatenate([s.target(k).get_chain(t=None).reshape(6, -1, 6) for k in range(2)], axis=1)
    assert np.array_equal(s._series.read(0, 6), rows)
    dens = np.concatenate([np.stack([s.target(k).get_log_like(t=None).reshape(6, -1), s.target(k).get_log_prior(t=None).reshape(6, -1)], axis=2)
                           for k in range(2)], axis=1)
    assert np.array_equal(s._dens.read(0, 6), dens)
    for k, eng in enumerate(members):
        same_run(s.target(k), first[k], plain.target(k), fp[k])
        one = solo_of(eng, counts[k], 6, betas[k], seeds[k], autocorr='device')
        two_runs(one, p0s[k])
        a = s.target(k)
        for t in (0, T - 1, None):
            got, want = a.get_summary(t=t, discard=1, thin=2), one.get_summary(t=t, discard=1, thin=2)
            assert sorted(got) == sorted(want) and all(np.array_equal(got[n], want[n]) for n in got), (k, t)
            tau, tau1 = a.get_autocorr_time(t=t, quiet=True), one.get_autocorr_time(t=t, quiet=True)
            assert tau.shape == tau1.shape and tau.tobytes() == tau1.tobytes(), (k, t, tau, tau1)
        assert np.array_equal(a.get_summary(t=0)['quantiles'], np.quantile(a.get_chain(flat=True), (0.16, 0.5, 0.84), axis=0).T)
        for method in ('ti', 'ss'):
            ev, ev1 = a.log_evidence(blocks=2, method=method), one.log_evidence(blocks=2, method=method)
            assert ev.log_z == ev1.log_z and ev.mc_error == ev1.mc_error and ev.ladder_error == ev1.ladder_error, (k, method, ev, ev1)
            assert np.array_equal(ev.mean_log_like, ev1.mean_log_like) and np.isfinite(ev.log_z)
        assert np.array_equal(a.mean_log_like(discard=2), one.mean_log_like(discard=2))
    grp.close()


def test_products_of_every_target():
    """Two targets on the products fixture's engine (a context may stand for several members): each target's derived columns
    from the one series equal its solo device run's."""
    from mcmc_spec_amd import synth
    from mcmc_spec_amd.group import TargetGroup
    from test_gpu_products import PRODUCT_COLS, engine
    eng = engine('B')
    c = common.golden_case('B')
    counts, T = [16, 12], 2
    betas, seeds = [[1.0, 0.4], [1.0, 0.6]], [5, 6]
    p0s = [synth.draw_walkers(T * n, seed=9 + k, tmin=c.tmin, tmax=c.tmax).reshape(T, n, 6) for k, n in enumerate(counts)]
    grp = TargetGroup([eng, eng])
    s = group_of(grp, counts, 6, betas, seeds, autocorr='device')
    s.run_mcmc(p0s, 9)
    for k in range(2):
        one = solo_of(eng, counts[k], 6, betas[k], seeds[k], autocorr='device')
        one.run_mcmc(p0s[k], 9)
        assert np.array_equal(s.target(k).get_chain(t=None), one.get_chain(t=None))
        for t in (1, None):
            got, want = s.target(k).get_products(PRODUCT_COLS, t=t, discard=1, thin=2), one.get_products(PRODUCT_COLS, t=t, discard=1, thin=2)
            assert all(np.array_equal(got[n], want[n]) for n in want) and np.all(np.isfinite(got['quantiles'])), (k, t)
    grp.close()


# ---- 8. prior rejection and errors ---------------------------------------------------------------------------------------------------
def doctored_run(find, K_hot=(1, 2)):
    """A host-drawn group run of ONE iteration on two targets whose first chunk carries one doctored stretch entry: in the first
    half-step of rung ``hot`` of target ``k``, the first entry j and factor z for which ``find(status_prior, status_like)`` holds
    at the proposal.  (sampler, twin draws per target, p0s, (k, hot, w), the engines)."""
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.group import TargetGroup
    from mcmc_spec_amd.moves import StretchMove
    c, engines = mixed_engines('B')
    members, counts, T = [engines[0], engines[5]], [12, 18], 3        # (target 1: the grid without its '3800, 5.0' node)
    betas, seeds = [1.0, 0.5, 0.25], [41, 42]
    shift = [0.0, 100.0]                                               # (target 1 starts above 3,900 K: no bracket needs the node)
    p0s = [inside(e, c, T * n, 90 + k, shift=shift[k]).reshape(T, n, 6) for k, (e, n) in enumerate(zip(members, counts))]
    grp = TargetGroup(members)
    s = group_of(grp, counts, 6, betas, seeds, rng='host', moves=StretchMove)
    arrays = group_of(grp, counts, 6, betas, seeds, rng='host', moves=StretchMove)._draw_members(1)   # the same generators: the same chunk
    sidx, cidx, kind, p1, p2, g, fac, logu = arrays
    k, hot = K_hot
    ctx = members[k].ctx
    a0 = sum(T * n // 2 for n in counts[:k]) + hot * (counts[k] // 2)   # the member's first entry in a half-step
    found = None
    for j in range(counts[k] // 2):
        sw = p0s[k][hot, sidx[0, 0, a0 + j]]
        cw = p0s[k][hot, cidx[0, 0, a0 + p1[0, 0, a0 + j]]]
        for z in np.concatenate([np.linspace(1.2, 12.0, 55), [20.0, 50.0, 100.0, 200.0, 500.0]]):
            for zz in (z, 1.0 / z):
                q = (cw - (cw - sw) * zz)[None]
                (_, st_p), (_, st_l) = ctx.logprob_batch(q, _lib.MODE_LOGPRIOR), ctx.logprob_batch(q, _lib.MODE_LOGLIKE)
                if find(int(st_p[0]), int(st_l[0])):
                    found = (j, zz, int(st_l[0]))
                    break
            if found:
                break
        if found:
            break
    assert found is not None
    j, z, code = found
    print('target', k, 'rung', hot, 'entry', j, 'factor', z, 'likelihood status', code)
    g[0, 0, a0 + j], fac[0, 0, a0 + j], logu[0, 0, a0 + j] = z, 5.0 * np.log(z), -1e300   # (any finite density would be accepted)
    s._draw_members = lambda m: [x[:m] for x in arrays]
    s._draw_swaps = lambda m: [np.full((m, sum((T - 1) * n for n in counts)), 1e300)]        # no swaps: the walker is found where it was
    return s, grp, arrays, p0s, (k, hot, int(sidx[0, 0, a0 + j])), members, counts, betas, code


def test_a_proposal_outside_the_prior_is_rejected_whatever_the_likelihood_reports():
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.tempered import TemperedSampler
    s, grp, arrays, p0s, (k, hot, w), members, counts, betas, _ = doctored_run(lambda sp, sl: sp == _lib.W_REJECT and sl > _lib.W_REJECT)
    s.run_mcmc(p0s, 1)
    a = s.target(k)
    assert np.array_equal(a.get_chain(t=hot)[0, w], p0s[k][hot, w]) and a.acceptance_fraction[hot, w] == 0
    assert a.acceptance_fraction.sum() > 0 and np.all(a.swap_fraction == 0)
    # the host loop under the same draws: the same rule, the same chain -- for both targets
    T, off = 3, 0
    for kk, (eng, n) in enumerate(zip(members, counts)):
        ns = n // 2
        mem = []
        for t in range(T):
            sl = slice(off + t * ns, off + (t + 1) * ns)
            mem.append(tuple(x[:, kk * T + t] if i == 2 else x[:, :, sl] for i, x in enumerate(arrays)))
        off += T * ns
        host = TemperedSampler(n, 6, eng, betas=betas, seeds=s.target(kk).seeds, draws=lambda i, m, mem=mem, n=n: (mem, np.full((1, T - 1, n), 1e300)))
        host.run_mcmc(p0s[kk], 1)
        b = s.target(kk)
        assert np.array_equal(host.get_chain(t=None), b.get_chain(t=None)) and np.array_equal(host.get_log_like(t=None), b.get_log_like(t=None))
        assert np.array_equal(host.get_log_prior(t=None), b.get_log_prior(t=None)) and np.array_equal(host.acceptance_fraction, b.acceptance_fraction)
    grp.close()


def test_a_walker_error_names_its_target():
    """Target 1's grid lacks a node: a proposal the prior admits whose bracket needs it is an error of the likelihood, raised
    with the target's name; the other target's rows of the chunk are not stored either (the run ends there)."""
    from mcmc_spec_amd import _lib
    s, grp, *_ = doctored_run(lambda sp, sl: sp == _lib.W_OK and sl > _lib.W_REJECT)
    with pytest.raises((KeyError, IndexError, ValueError), match='target 1: '):
        s.run_mcmc(_[1], 1)
    assert len(s.target(0).get_chain()) == 0 == len(s.target(1).get_chain())
    grp.close()


# ---- 9. refusals through the ABI ---------------------------------------------------------------------------------------------------
def test_refusals_through_the_abi():
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd.group import TargetGroup
    from mcmc_spec_amd.moves import parse_moves
    from mcmc_spec_amd.sampler import EnsembleSampler
    from mcmc_spec_amd.tempered import draw_swap_logu, swap_generator
    c = common.golden_case('B')
    a, b = Engine(0), Engine(0)
    for e in (a, b):
        e.stage_specs(c.specs)
        _stage(e, c)
    counts, T = [12, 18], 3
    W = T * sum(counts)
    betas = np.array([[1.0, 0.5, 0.25], [1.0, 0.4, 0.1]])
    seeds = [[7, 8, 9], [70, 80, 90]]
    pk = [inside(e, c, T * n, 20 + k) for k, (e, n) in enumerate(zip((a, b), counts))]
    p0 = np.concatenate(pk)
    lpr = np.concatenate([e.ctx.logprob_batch(p, _lib.MODE_LOGPRIOR)[0] for e, p in zip((a, b), pk)])
    ll = np.concatenate([e.ctx.logprob_batch(p, _lib.MODE_LOGLIKE)[0] for e, p in zip((a, b), pk)])
    grp = TargetGroup([a, b])
    g = grp.group

    def raises(code, fn, *args, **kw):
        with pytest.raises(_lib.MsxError) as ei:
            fn(*args, **kw)
        assert ei.value.code == code, ei.value

    def begin(betas=betas, counts=counts, coords=p0, ll=ll, lpr=lpr, grp=g, steps=2):
        grp.tempered_begin(betas, counts, coords, ll, lpr, steps)

    def nothing_queued():
        for slot in (0, 1):
            raises(_lib.MSX_ERR_STATE, g.tempered_collect, slot, 2)

    # ---- begin: MSX_ERR_INVALID ----
    raises(_lib.MSX_ERR_INVALID, lambda: g.check(g.lib.msx_group_tempered_begin(
        g.h, 0, _lib.dptr(betas), _lib.iptr(np.array(counts, dtype=np.int64)), 6, 2, _lib.dptr(p0), _lib.dptr(ll), _lib.dptr(lpr))))   # no rungs
    n33 = 33 * sum(counts)
    raises(_lib.MSX_ERR_INVALID, begin, betas=np.tile(np.geomspace(1.0, 0.01, 33), (2, 1)), coords=np.resize(p0, (n33, 6)),
           ll=np.resize(ll, n33), lpr=np.resize(lpr, n33))                                    # 2 x 33 members
    for row in ([1.0, 0.5, 0.5], [0.5, 1.0, 2.0], [1.0, 0.5, 0.0], [1.0, 0.5, -0.1], [1.0, float('nan'), 0.1], [float('inf'), 1.0, 0.5]):
        raises(_lib.MSX_ERR_INVALID, begin, betas=np.array([betas[0], row]))                  # target 1's ladder
    odd = [12, 17]
    n = T * sum(odd)
    raises(_lib.MSX_ERR_INVALID, begin, counts=odd, coords=p0[:n], ll=ll[:n], lpr=lpr[:n])    # an odd count
    raises(_lib.MSX_ERR_INVALID, begin, counts=[0, 18], coords=p0[:54], ll=ll[:54], lpr=lpr[:54])   # a count below 2
    bad = lpr.copy()
    bad[40] = -np.inf
    raises(_lib.MSX_ERR_INVALID, begin, lpr=bad)                                              # outside the prior at the start
    bad = ll.copy()
    bad[W - 1] = np.nan
    raises(_lib.MSX_ERR_INVALID, begin, ll=bad)
    raises(_lib.MSX_ERR_INVALID, begin, coords=np.zeros((W, 8)))                              # ndim
    # ---- begin: MSX_ERR_STATE ----
    a.ctx.sampler_begin(_lib.MODE_LOGPOST, pk[0][:12], lpr[:12] + ll[:12], 2)
    raises(_lib.MSX_ERR_STATE, begin)                                                         # a member's context runs its own sampler
    a.ctx.sampler_end()
    b.ctx.sampler_policy(0)
    b.ctx.tempered_begin(betas[1], pk[1].reshape(T, 18, 6), ll[36:].reshape(T, 18), lpr[36:].reshape(T, 18), 2)
    raises(_lib.MSX_ERR_STATE, begin)                                                         # ... or its own ladder
    b.ctx.tempered_end()
    b.ctx.sampler_policy(-1)
    g.sampler_begin(_lib.MODE_LOGPOST, p0[:30], (lpr + ll)[:30], [12, 18], 2)
    raises(_lib.MSX_ERR_STATE, begin)                                                         # the group's sampler in flight
    g.sampler_end()
    ranks = [Engine(0) for _ in range(2)]
    for e in ranks:
        e.stage_specs(c.specs)
        _stage(e, c)
    with_comm = TargetGroup(ranks)
    _lib.Context.comm_init_loopback([e.ctx for e in ranks])
    raises(_lib.MSX_ERR_STATE, begin, grp=with_comm.group)                                    # a member holds a communicator
    with_comm.close()
    # ---- a run: refused calls queue nothing ----
    begin()
    raises(_lib.MSX_ERR_STATE, begin)                                                         # a tempered run in flight
    raises(_lib.MSX_ERR_STATE, g.sampler_begin, _lib.MODE_LOGPOST, p0[:30], (lpr + ll)[:30], [12, 18], 2)   # ... refuses the other family
    for lag, time in ((0.0, 1.0), (float('inf'), 1.0), (10.0, 0.5), (10.0, float('nan'))):
        raises(_lib.MSX_ERR_INVALID, g.tempered_adapt, [10.0, lag], [1.0, time], [0, 0])
    raises(_lib.MSX_ERR_INVALID, g.tempered_adapt, [10.0, 10.0], [1.0, 1.0], [0, -1])
    members = [n for n in counts for _ in range(T)]
    chain_s, dens_s = _lib.Series(a.ctx, W, 6, members), _lib.Series(a.ctx, W, 2, members)
    wrong = _lib.Series(a.ctx, W, 6, [T * n for n in counts])                                 # K members, not K T
    raises(_lib.MSX_ERR_INVALID, g.tempered_attach_series, wrong, dens_s, 0)
    raises(_lib.MSX_ERR_INVALID, g.tempered_attach_series, chain_s, chain_s, 0)
    raises(_lib.MSX_ERR_INVALID, g.tempered_attach_series, chain_s, dens_s, 1)                # past the rows held
    g.tempered_attach_series(chain_s, dens_s, 0)
    raises(_lib.MSX_ERR_STATE, g.tempered_attach_series, chain_s, dens_s, 0)                  # twice
    g.tempered_adapt([10.0, 10.0], [1.0, 1.0], [0, 0])
    raises(_lib.MSX_ERR_STATE, g.tempered_adapt, [10.0, 10.0], [1.0, 1.0], [0, 0])            # twice
    g.tempered_end()
    chain_s.close(), dens_s.close(), wrong.close()
    begin()
    rungs = [EnsembleSampler(n, 6, None, seed=s, moves=mix(), _general=True) for n, row in zip(counts, seeds) for s in row]
    swaps = [swap_generator(row[0]) for row in seeds]

    def chunk(m):
        per = [r._draw_steps(m) for r in rungs]
        out = [np.stack([p[i] for p in per], axis=1) if i == 2 else np.concatenate([p[i] for p in per], axis=2) for i in range(8)]
        return out + [np.concatenate([draw_swap_logu(sw, m, T, n).reshape(m, -1) for sw, n in zip(swaps, counts)], axis=1)]
    good = chunk(2)
    H0 = T * counts[0] // 2                    # target 1's first entry of a half-step

    def fed(code, arrays, slot=0):
        raises(code, g.tempered_enqueue, slot, *arrays)

    def drawn(code, slot=0, nsteps=2, sd=seeds, moves=None, first_iter=0):
        raises(code, g.tempered_enqueue_drawn, slot, nsteps, sd, mix() if moves is None else moves, first_iter)

    bad = [x.copy() for x in good]
    bad[2][1, 4] = 2                                   # an out-of-range kind (member 4: target 1, rung 1)
    fed(_lib.MSX_ERR_INVALID, bad)
    bad = [x.copy() for x in good]
    bad[2][:] = 1
    bad[4][0, 1, H0 + 3] = bad[3][0, 1, H0 + 3]        # p1 == p2 on a DE entry
    fed(_lib.MSX_ERR_INVALID, bad)
    bad = [x.copy() for x in good]
    bad[3][1, 0, H0] = 9                               # p1 past target 1's complementary half (9 walkers)
    fed(_lib.MSX_ERR_INVALID, bad)
    bad = [x.copy() for x in good]
    bad[0][0, 1, 2] = 12                               # a walker index past target 0's rung (12 walkers)
    fed(_lib.MSX_ERR_INVALID, bad)
    st = parse_moves(mix()).as_struct()
    st.weight[0] = 0.6                                 # weights that do not sum to 1
    drawn(_lib.MSX_ERR_INVALID, moves=st)
    drawn(_lib.MSX_ERR_INVALID, first_iter=-1)
    drawn(_lib.MSX_ERR_INVALID, nsteps=3)              # longer than the run's chunks
    drawn(_lib.MSX_ERR_INVALID, slot=2)                # no such slot
    nothing_queued()
    # a host-fed chunk then a drawn one, against the all-drawn run: the refused calls left nothing behind
    g.tempered_enqueue(0, *good)
    raises(_lib.MSX_ERR_STATE, g.tempered_adapt, [10.0, 10.0], [1.0, 1.0], [0, 0])            # after the first enqueue
    late = _lib.Series(a.ctx, W, 6, members)
    raises(_lib.MSX_ERR_STATE, g.tempered_attach_series, late, None, 0)
    late.close()
    drawn(_lib.MSX_ERR_STATE)                                                                 # slot not collected yet
    first = g.tempered_collect(0, 2)
    assert first[0].shape == (2, W, 6) and first[4].shape == (2, T - 1) and first[5].shape == (2, T) and not first[5].any()
    assert np.array_equal(g.tempered_betas(0, 2), np.tile(betas, (2, 1, 1)))                  # a fixed run: the begin ladders in every row
    lad = g.tempered_ladder()
    assert np.array_equal(lad[0], betas) and not lad[1].any() and not lad[2].any()
    end_fed = g.tempered_end(want_state=True)
    assert np.array_equal(end_fed[0], first[0][-1]) and np.array_equal(end_fed[1], first[1][-1])
    assert g.tempered_end() is None                                                           # no run: nothing to end
    raises(_lib.MSX_ERR_STATE, g.tempered_collect, 0, 2)
    drawn(_lib.MSX_ERR_STATE)
    # the fed chunk is what a DeviceGroupTemperedSampler(rng='host') queues: its solo twins walk it
    for k, (e, n) in enumerate(zip((a, b), counts)):
        one = solo_of(e, n, 6, betas[k], seeds[k], rng='host')
        one.run_mcmc(pk[k].reshape(T, n, 6), 2)
        sl = slice(T * sum(counts[:k]), T * sum(counts[:k + 1]))
        assert np.array_equal(first[0][:, sl].reshape(2, T, n, 6), one.get_chain(t=None))
        assert np.array_equal(first[1][:, sl].reshape(2, T, n), one.get_log_like(t=None))
    # more than 4,096 walkers per rung: begun, fed from the host if at all, never drawn
    big = [4098, 12]
    nb = sum(big)
    bp = np.concatenate([np.resize(pk[0][:1], (4098, 6)), pk[1][:12]])
    bl, bpr = np.concatenate([np.resize(ll[:1], 4098), ll[36:48]]), np.concatenate([np.resize(lpr[:1], 4098), lpr[36:48]])
    g.tempered_begin(np.ones((2, 1)), big, bp, bl, bpr, 2)
    raises(_lib.MSX_ERR_INVALID, g.tempered_enqueue_drawn, 0, 2, [[1], [2]], mix(), 0)
    raises(_lib.MSX_ERR_STATE, g.tempered_collect, 0, 2)
    assert g.tempered_end(want_state=True)[0].shape == (nb, 6)
    # ---- a member restaged mid-run: the next chunk is refused, then only end; the group is poisoned for good ----
    begin()
    g.tempered_enqueue_drawn(0, 2, seeds, mix(), 0)
    g.tempered_collect(0, 2)
    _stage(b, c)
    raises(_lib.MSX_ERR_STATE, g.tempered_enqueue_drawn, 1, 2, seeds, mix(), 2)               # staged again since msx_group_create
    raises(_lib.MSX_ERR_STATE, g.tempered_enqueue_drawn, 1, 2, seeds, mix(), 2)               # the run failed
    raises(_lib.MSX_ERR_STATE, g.tempered_collect, 0, 2)
    g.tempered_end()
    raises(_lib.MSX_ERR_STATE, begin)                                                         # restaged since create: at begin too
    grp.close()
    # a fresh group on the same engines is usable; a group closed with a run open ends it; a destroyed member is refused
    grp = TargetGroup([a, b])
    begin(grp=grp.group)
    grp.group.tempered_enqueue_drawn(0, 2, seeds, mix(), 0)
    again = grp.group.tempered_collect(0, 2)
    assert again[0].shape == (2, W, 6) and np.all(np.isfinite(again[1]))
    grp.close()
    grp = TargetGroup([a, b])
    a.ctx.close()
    raises(_lib.MSX_ERR_STATE, begin, grp=grp.group)
    grp.close()
