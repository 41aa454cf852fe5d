"""GPU: every logprior branch of the reference (tests/golden/golden_prior.npz, tests/golden/make_prior_golden.py) through
every form of the hot path -- fused, generic-recipe fused, pair, linked, in-path, target group -- and the device-resident
samplers with use_av off.  The gates and the prior terms are written once per form in the device code; this pins each
copy to the reference itself, not only to the others.

Status words follow the fixture's outcome codes (the gate's reject takes precedence over ValueError, as logprior runs
first in the reference); a triple with dist_fit and without rad_prior, where the reference returns None, has the
engine's value instead: the sum the reference's list holds at its `return`."""
import numpy as np
import pytest

import common
from common import golden_case, rel_err
from oracle import mft6_oracle as orc
from test_oracle_prior_branches import NEG_INF, NONE, OK, VALUEERROR, av_prior_of, prior_golden

pytestmark = pytest.mark.gpu
TIGHT = 1e-9


def _lib():
    from mcmc_spec_amd import _lib as L
    return L


def case_of(ndim):
    return golden_case('B' if ndim == 6 else 'C')


def av_table(g, table):
    return g['av%d_edges' % table], g['av%d_mu' % table], g['av%d_sig' % table]


def padded_av_table(g, table):
    """The same lookups from a table too large for the register-resident recipe: bins below the first edge repeat bin
    0, bins beyond the last repeat the last one (the clamp of mft6.py's stand-in gives those values there)."""
    e, mu, sig = av_table(g, table)
    lo, hi = np.linspace(0.5, e[0], 41)[:-1], np.linspace(e[-1], 20000.0, 41)[1:]
    return (np.concatenate([lo, e, hi]), np.concatenate([np.full(40, mu[0]), mu, np.full(40, mu[-1])]),
            np.concatenate([np.full(40, sig[0]), sig, np.full(40, sig[-1])]))


def flags(g, ndim, combo):
    df, ext, rp, hp = (bool(x) for x in g['combos%d' % ndim][combo])
    return dict(dist_fit=df, use_av=ext, rad_prior=rp, prior=list(g['prior%d' % ndim]) if hp else 0)


def stage(eng, g, ndim, combo, table, box, data=None, av=None):
    from mcmc_spec_amd import bands
    c = case_of(ndim)
    d = data or dict(data=c.data, err=c.err, fr=c.fr, r=c.r, ctm=c.ctm, ptm=c.ptm, tmi=c.tmi, tma=c.tma)
    eng.stage_problem(d['data'], d['err'], d['fr'], d['r'], d['ctm'], d['ptm'], d['tmi'], d['tma'], c.matrix,
                      nspec=c.nspec, bands=bands.make_bands(c.tables, *c.vega),
                      av_table=av if av is not None else av_table(g, table), tmin=g['tmin'][box], tmax=g['tmax'][box],
                      **flags(g, ndim, combo))


def golden_engine():
    from mcmc_spec_amd.engine import Engine
    if 'prior_branches' not in common._cache:
        eng = Engine(0)
        eng.stage_specs(golden_case('B').specs)
        common._cache['prior_branches'] = eng
    return common._cache['prior_branches']


def fall_through_value(t, ndim, ext, prior, avp):
    """The triple with dist_fit and without rad_prior: the sum of the reference's `pp` where its `return` would be
    (mft6.py:1358-1381): the A_V term and the Gaussian list."""
    ns = (ndim - 2) // 2
    pp = []
    if ext:
        mu, sig = avp(1.0 / t[2 * ns + 1])
        pp.append(-0.5 * ((t[ns] - mu) / (0.05 if sig == 0 else sig)) ** 2)
    if prior != 0:
        ps = prior[:ns] + [prior[2 * ns]] + prior[2 * ns + 2:3 * ns + 2] + [prior[-2]]
        ss = prior[ns:2 * ns] + [prior[2 * ns + 1]] + prior[3 * ns + 2:4 * ns + 2] + [prior[-1]]
        pp += [-0.5 * ((t[k] - p) / ss[k]) ** 2 for k, p in enumerate(ps) if p != 0]
    return np.sum(pp)


def expected_prior(g, ndim, table, combo, sel):
    """(status, value) per walker of `sel` in MODE_LOGPRIOR."""
    L = _lib()
    code, lp = g['code%d' % ndim][table, combo, sel], g['lp%d' % ndim][table, combo, sel].copy()
    st = np.select([code == OK, code == NEG_INF, code == NONE, code == VALUEERROR],
                   [L.W_OK, L.W_REJECT, L.W_OK, L.W_VALUEERROR], -1)
    assert np.all(st >= 0)
    f = flags(g, ndim, combo)
    for j in np.nonzero(code == NONE)[0]:
        lp[j] = fall_through_value(g['theta%d' % ndim][sel][j], ndim, f['use_av'], f['prior'], av_prior_of(g, table))
    return st, lp


_LL = {}


def oracle_ll(ndim, ext, i, t):
    """(status, value) of the oracle's log-likelihood of walker i (cached: it depends on ndim, ext and theta alone)."""
    L = _lib()
    key = (ndim, ext, i)
    if key not in _LL:
        c = case_of(ndim)
        try:
            _LL[key] = (L.W_OK, orc.loglikelihood(list(t), c.fr, c.nspec, c.data, c.err, c.r, c.specs, c.ctm, c.ptm,
                                                  c.tmi, c.tma, c.matrix, av=ext, bandlib=c.bandlib))
        except KeyError:
            _LL[key] = (L.W_KEYERROR, np.nan)
        except IndexError:
            _LL[key] = (L.W_INDEXERROR, np.nan)
        except ValueError:
            _LL[key] = (L.W_VALUEERROR, np.nan)
    return _LL[key]


def expected_post(g, ndim, table, combo, sel, pst, plp):
    L = _lib()
    ext = bool(g['combos%d' % ndim][combo][1])
    st, v = pst.copy(), np.where(pst == L.W_REJECT, -np.inf, np.nan)
    for j, i in enumerate(np.nonzero(sel)[0]):
        if pst[j] == L.W_OK:
            s, ll = oracle_ll(ndim, ext, i, g['theta%d' % ndim][i])
            st[j] = s
            v[j] = plp[j] + ll if s == L.W_OK else np.nan
    return st, v


def check(st, lp, want_st, want_lp, what):
    assert np.array_equal(st, want_st), (what, np.nonzero(st != want_st)[0], st[st != want_st], want_st[st != want_st])
    ok = want_st == 0
    assert np.array_equal(np.isneginf(lp[ok]), np.isneginf(want_lp[ok])), what
    fin = ok & np.isfinite(want_lp)
    assert np.all(np.isfinite(lp[fin])) and rel_err(lp[fin], want_lp[fin]).max(initial=0.0) < TIGHT, what


def run(eng, th, mode, path=None):
    L = _lib()
    eng.ctx.set_path(L.PATH_FUSED if path is None else path)
    try:
        return eng.ctx.logprob_batch(np.ascontiguousarray(th), mode)
    finally:
        eng.ctx.set_path(L.PATH_AUTO)


def same_bits(a, b):
    return np.array_equal(a[0], b[0], equal_nan=True) and np.array_equal(a[1], b[1])


@pytest.mark.parametrize('table', [0, 1])
@pytest.mark.parametrize('ndim', [6, 8])
def test_fused_generic_and_pair_forms_against_the_reference(ndim, table):
    """Every combination: the fused form against the fixture (prior) and fixture prior + oracle log-likelihood
    (posterior); the generic recipe (a padded A_V table: the same lookups) against the same, to TIGHT (its arithmetic
    is its own: plain divisions where the register-resident recipe has fast_div); for binaries, the pair form
    (>= 2,048 walkers) gives the fused form's bits."""
    L = _lib()
    g = prior_golden()
    eng = golden_engine()
    th_all, boxes = g['theta%d' % ndim], g['tbox%d' % ndim]
    for combo in range(len(g['combos%d' % ndim])):
        for box in (0, 1):
            sel = boxes == box
            th = th_all[sel]
            what = (ndim, table, tuple(int(x) for x in g['combos%d' % ndim][combo]), box)
            stage(eng, g, ndim, combo, table, box)
            pst, plp = expected_prior(g, ndim, table, combo, sel)
            lp_prior, st_prior = run(eng, th, L.MODE_LOGPRIOR)
            check(st_prior, lp_prior, pst, plp, what + ('prior',))
            fused = run(eng, th, L.MODE_LOGPOST)
            wst, wlp = expected_post(g, ndim, table, combo, sel, pst, plp)
            check(fused[1], fused[0], wst, wlp, what + ('post',))
            if ndim == 6:
                reps = -(-2048 // len(th))
                big = np.tile(th, (reps, 1))
                pair = run(eng, big, L.MODE_LOGPOST, L.PATH_PAIR)
                assert eng.ctx.last_form() == L.FORM_PAIR, what
                assert same_bits(pair, (np.tile(fused[0], reps), np.tile(fused[1], reps))), what + ('pair',)
            stage(eng, g, ndim, combo, table, box, av=padded_av_table(g, table))
            gen_prior = run(eng, th, L.MODE_LOGPRIOR)
            check(gen_prior[1], gen_prior[0], pst, plp, what + ('generic prior',))
            gen = run(eng, th, L.MODE_LOGPOST)
            check(gen[1], gen[0], wst, wlp, what + ('generic post',))


@pytest.mark.parametrize('ndim', [6, 8])
def test_group_launch_members_differ_only_in_prior_flags(ndim):
    """One target-group launch per A_V table whose members are the 16 flag combinations x the two Teff boxes: each
    member's walkers get the bits of its own fused launch, and those are the reference's."""
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd.group import TargetGroup
    L = _lib()
    g = prior_golden()
    ncombo = len(g['combos%d' % ndim])
    key = 'prior_branches_group'
    if key not in common._cache:
        engs = []
        for _ in range(2 * ncombo):
            e = Engine(0)
            e.stage_specs(golden_case('B').specs)
            engs.append(e)
        common._cache[key] = engs
    engs = common._cache[key]
    th_all, boxes = g['theta%d' % ndim], g['tbox%d' % ndim]
    for table in (0, 1):
        members = [(combo, box) for combo in range(ncombo) for box in (0, 1)]
        for e, (combo, box) in zip(engs, members):
            stage(e, g, ndim, combo, table, box)
        grp = TargetGroup(engs)
        thetas = [th_all[boxes == box] for _, box in members]
        counts = np.array([len(t) for t in thetas], dtype=np.int64)
        for mode in (L.MODE_LOGPRIOR, L.MODE_LOGPOST):
            logp, status = grp.group.logprob_batch(np.concatenate(thetas), counts, mode)
            o = 0
            for e, t, (combo, box) in zip(engs, thetas, members):
                what = (ndim, table, combo, box, mode)
                solo = run(e, t, mode)
                assert same_bits((logp[o:o + len(t)], status[o:o + len(t)]), solo), what
                if mode == L.MODE_LOGPRIOR:
                    pst, plp = expected_prior(g, ndim, table, combo, boxes == box)
                    check(solo[1], solo[0], pst, plp, what)
                o += len(t)
        grp.close()


def test_reference_posteriors():
    """The stored reference logposterior values (golden case B, and C for the triple) through the engine; where the
    reference raised TypeError the engine has a finite value."""
    L = _lib()
    g = prior_golden()
    eng = golden_engine()
    from mcmc_spec_amd import bands
    for ndim in (6, 8):
        c = case_of(ndim)
        th = g['post%d_theta' % ndim]
        for ci, (df, ext, rp) in enumerate(g['post%d_combos' % ndim]):
            eng.stage_problem(c.data, c.err, c.fr, c.r, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=c.nspec,
                              bands=bands.make_bands(c.tables, *c.vega), av_table=av_table(g, 0), tmin=c.tmin, tmax=c.tmax,
                              prior=list(g['prior%d' % ndim]), use_av=bool(ext), dist_fit=bool(df), rad_prior=bool(rp))
            lp, st = run(eng, th, L.MODE_LOGPOST)
            code, want = g['post%d_code' % ndim][ci], g['post%d_value' % ndim][ci]
            what = (ndim, df, ext, rp)
            assert np.array_equal(st[code != 4], np.where(code == NEG_INF, L.W_REJECT, L.W_OK)[code != 4]), what
            assert np.array_equal(np.isneginf(lp), code == NEG_INF), what
            fin = code == OK
            assert rel_err(lp[fin], want[fin]).max(initial=0.0) < TIGHT, what
            assert np.all(np.isfinite(lp[code == 4])) and np.all(st[code == 4] == L.W_OK), what


def wide_workload(key, npix, broaden):
    from bench import build_workload
    from mcmc_spec_amd.engine import Engine
    if key not in common._cache:
        eng = Engine(0)
        W = build_workload(eng, npix, True, broaden=broaden)
        common._cache[key] = (eng, W)
    return common._cache[key]


@pytest.mark.parametrize('form', ['linked', 'in_path'])
def test_linked_and_inpath_forms_on_every_binary_combination(form):
    """Binaries on the benchmark's synthetic workload: 16,384 px (the linked form, one workgroup per 8,192-px segment)
    and 4,096 px with the broadening in the walker's path.  The prior against the fixture; the posterior's statuses and
    -inf sets against the fused form's, its values to the fused form's bits (linked) or 1e-11 (in-path: the broadening
    is summed in another order)."""
    L = _lib()
    g = prior_golden()
    ndim = 6
    eng, W = wide_workload('prior_linked', 16384, 'staging') if form == 'linked' else \
        wide_workload('prior_inpath', 4096, 'in_path')
    path = L.PATH_LINKED if form == 'linked' else L.PATH_INPATH
    data = {k: W[k] for k in ('data', 'err', 'fr', 'r', 'ctm', 'ptm', 'tmi', 'tma')}
    th_all, boxes = g['theta6'], g['tbox6']
    for table in (0, 1):
        for combo in range(len(g['combos6'])):
            for box in (0, 1):
                sel = boxes == box
                th = th_all[sel]
                what = (form, table, combo, box)
                stage(eng, g, ndim, combo, table, box, data=data)
                pst, plp = expected_prior(g, ndim, table, combo, sel)
                pr = run(eng, th, L.MODE_LOGPRIOR)  # (MODE_LOGPRIOR has no spectrum pass: the fused form only)
                check(pr[1], pr[0], pst, plp, what + ('prior',))
                fused = run(eng, th, L.MODE_LOGPOST)
                other = run(eng, th, L.MODE_LOGPOST, path)
                assert np.array_equal(other[1], fused[1]) and np.array_equal(np.isneginf(other[0]), np.isneginf(fused[0])), what
                assert np.array_equal(fused[1][pst == L.W_REJECT], pst[pst == L.W_REJECT]), what
                if form == 'linked':
                    assert same_bits(other, fused), what
                else:  # (values where both Teffs lie on the workload's grid: outside it the bracket wraps to the far node)
                    fin = np.isfinite(fused[0]) & np.all((th[:, :2] >= W['tmin']) & (th[:, :2] <= W['tmax']), axis=1)
                    assert rel_err(other[0][fin], fused[0][fin]).max(initial=0.0) < 1e-11, what


def _chain_start(nw, rng):
    p0 = np.array([3850.0, 3025.0, 0.45, 0.5, 0.31, 2.0732e-3]) + rng.normal(size=(nw, 6)) * np.array(
        [30, 30, 0.005, 0.02, 0.02, 2e-5])
    p0[:, 1] = np.clip(p0[:, 1], 3001.0, None)
    return p0


def test_device_resident_chains_without_extinction_against_the_oracle_stretch_move():
    """use_av off, dist_fit and rad_prior on (the radius prior reads [A_V, R1] as the reference does): the
    device-resident sampler, and one member of a device-resident group beside a use_av member, against
    oracle/stretch_move.py driving the oracle's logposterior from the same random numbers."""
    from oracle import stretch_move as osm
    from mcmc_spec_amd import bands
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler, EnsembleSampler
    c = golden_case('B')
    g = prior_golden()
    bl = bands.make_bands(c.tables, *c.vega)

    def staged(use_av):
        e = Engine(0)
        e.stage_specs(c.specs)
        e.stage_problem(c.data, c.err, c.fr, c.r, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=2, bands=bl,
                        av_table=av_table(g, 0), tmin=c.tmin, tmax=c.tmax, prior=c.prior, use_av=use_av, rad_prior=True)
        return e
    avp = av_prior_of(g, 0)
    f = lambda q: np.array([orc.logposterior(list(t), c.fr, 2, c.data, c.err, c.r, c.specs, c.ctm, c.ptm, c.tmi, c.tma,  # noqa: E731
                                             c.tmin, c.tmax, c.matrix, avp, prior=c.prior, a=False, rad_prior=True,
                                             bandlib=c.bandlib) for t in q])
    nw, nsteps = 16, 8
    rng = np.random.default_rng(5)
    off, on = staged(False), staged(True)
    p0 = _chain_start(nw, rng)
    assert np.all(np.isfinite(f(p0)))

    def oracle_chain(seed):
        twin = EnsembleSampler(nw, 6, None, vectorize=True, seed=seed)
        sidx, cidx, partner, zz, zfac, logu = twin._draw_steps(nsteps)
        return osm.run_chain(p0, f(p0), (sidx, cidx, partner, zz, logu), f)

    dev = DeviceEnsembleSampler(nw, 6, off, seed=17, chunk=4)
    dev.run_mcmc(p0, nsteps)
    chain, lpc, nacc = oracle_chain(17)
    assert np.array_equal(dev.get_chain(), chain)
    assert rel_err(dev.get_log_prob(), lpc).max() < TIGHT
    assert np.array_equal(dev.acceptance_fraction, nacc / nsteps) and 0 < nacc.sum() < nw * nsteps

    grp = TargetGroup([on, off])
    seeds = [23, 29]
    p0_on = _chain_start(nw, np.random.default_rng(6))
    gs = DeviceGroupSampler([nw, nw], 6, grp, seeds=seeds, chunk=3)
    gs.run_mcmc([p0_on, p0], nsteps)
    chain, lpc, nacc = oracle_chain(29)
    assert np.array_equal(gs.get_chain(1), chain)
    assert rel_err(gs.get_log_prob(1), lpc).max() < TIGHT
    assert np.array_equal(gs.acceptance_fraction[1], nacc / nsteps)
    grp.close()


def test_dropins_follow_the_reference_where_it_returns_none_and_without_extinction():
    """The drop-in signatures (mcmc_spec_amd/mft6.py): a triple with dist_fit and without rad_prior gives None from
    logprior for walkers inside the gates (an object array for a batch) and TypeError from logposterior and
    device_sampler, as the reference does (mft6.py:1383-1393, :1465); logprior(ext=False) / logposterior(a=False) on a
    binary against the reference's posteriors and the oracle's prior."""
    import mcmc_spec_amd.mft6 as m
    from mcmc_spec_amd import bands
    g = prior_golden()
    c = golden_case('C')
    m.clear_cache()
    m.set_band_library(bands.make_bands(c.tables, *c.vega))
    m.set_av_prior(*av_table(g, 0))
    th = g['post8_theta']
    bad = th[0].copy()
    bad[0] = 2999.0  # outside the Teff box: -inf before the fall-through
    args = [c.fr, 3, 0, c.data, c.err, 1700, c.r, c.specs, c.ctm, c.ptm, c.tmi, c.tma, None, c.tmin, c.tmax, c.matrix,
            10.0, 20.0]
    prior = list(g['prior8'])
    with pytest.raises(TypeError):
        m.logposterior(th, *args, prior=prior)
    with pytest.raises(TypeError):
        m.logposterior(th[0], *args, prior=prior, a=False)
    assert m.logposterior(bad, *args, prior=prior) == -np.inf
    assert m.logprior(th[0], 3, 0, c.tmin, c.tmax, c.matrix, 10.0, 20.0, prior=prior) is None
    lp = m.logprior(np.vstack([th, bad]), 3, 0, c.tmin, c.tmax, c.matrix, 10.0, 20.0, prior=prior)
    assert lp.dtype == object and list(lp) == [None] * len(th) + [-np.inf]
    with pytest.raises(TypeError):
        m.device_sampler(16, 8, args, dict(prior=prior))
    combos = [tuple(int(x) for x in k) for k in g['post8_combos']]
    want = g['post8_value'][combos.index((1, 1, 1))]
    assert rel_err(m.logposterior(th, *args, prior=prior, rad_prior=True), want).max() < TIGHT
    m.device_sampler(16, 8, args, dict(prior=prior, rad_prior=True))  # a value there: accepted
    # the binary without extinction
    c = golden_case('B')
    th = g['post6_theta']
    args = [c.fr, 2, 0, c.data, c.err, 1700, c.r, c.specs, c.ctm, c.ptm, c.tmi, c.tma, None, c.tmin, c.tmax, c.matrix,
            10.0, 20.0]
    prior = list(g['prior6'])
    avp = av_prior_of(g, 0)
    for ci, (df, ext, rp) in enumerate(g['post6_combos']):
        if ext:
            continue
        kw = dict(prior=prior, dist_fit=bool(df), rad_prior=bool(rp))
        got = m.logposterior(th, *args, a=False, **kw)
        code, want = g['post6_code'][ci], g['post6_value'][ci]
        assert np.array_equal(np.isneginf(got), code == NEG_INF) and rel_err(got[code == OK], want[code == OK]).max() < TIGHT
        lp = m.logprior(th, 2, 0, c.tmin, c.tmax, c.matrix, 10.0, 20.0, ext=False, **kw)
        wantp = np.array([orc.logprior(list(t), 2, c.tmin, c.tmax, c.matrix, avp, ext=False, **kw) for t in th])
        assert np.array_equal(np.isneginf(lp), np.isneginf(wantp)) and rel_err(lp, wantp).max() < TIGHT
    m.clear_cache()
