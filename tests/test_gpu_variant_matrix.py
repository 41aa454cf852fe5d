"""GPU: every compiled instance of the hot kernel, by name.  For each recipe of tests/variant_cases.py -- one per entry of
kVariants, kPairVariants and kGroupVariants (tests/test_variant_cases.py holds the table to the source) -- a synthetic
problem on the golden grid is staged, the planner is asked and must answer the instance the case names (a recipe that no
longer reaches its instance FAILS, naming it; it never skips), and a batch tiled from eight probe walkers is evaluated in
the three value modes with the case's workgroup size and path:

* statuses equal the reference instance's (256 threads, fused form, the eight probes alone), finiteness the oracle's;
* every copy of a probe in the batch -- the first eight and the last eight positions, both sides of a sub-batch boundary
  where the form has one -- carries the same bits;
* finite values agree with oracle/mft6_oracle.py to 1e-9 relative (float32-stored R table: BASELINE.json's 1e-6);
* the bits are the reference instance's (the in-path form, another placement of the broadening: 1e-11 against it).

And the group's device-resident sampler on every SMP instance the automatic plan reaches, and on every neighbour it
substitutes for an entry built without one: three iterations, bit for bit GroupSampler's chain.

Each parametrised case prints the kernel that ran and its largest relative deviation from the oracle."""
import os

import numpy as np
import pytest

import common
import variant_cases as vc
from common import golden_case, rel_err

pytestmark = pytest.mark.gpu

TIGHT = 1e-9          # tests/test_gpu_parity.py: what float64 with re-ordered sums should easily meet
BASELINE_TOL = 1e-6   # BASELINE.json: "chi^2 matching CPU reference to <= 1e-6 rel" (tests/test_gpu_f32_storage.py)
INPATH_TOL = 1e-11    # tests/test_gpu_inpath.py: the in-path form against the staging placement
RESOLUTION = 1700.0
SWITCHES = ('MSX_LINKED', 'MSX_PAIR_MIN', 'MSX_SCRATCH_MB', 'MSX_INPATH_MB')   # they move what a recipe reaches
MODES = ('LOGLIKE', 'LOGPOST', 'CHISQ')


def _no_switches():
    found = [k for k in SWITCHES if k in os.environ]
    if found:
        pytest.skip('%s set in the environment: the planner is not the one the recipes were written for' % ', '.join(found))


def _case(nspec):
    return golden_case('B' if nspec == 2 else 'C')


def _window(r):
    return [float(r[0]) * 1e4 - 2.0, float(r[1]) * 1e4 + 2.0]


def problem(nspec, npix, store='f64', broadening='staging'):
    """The staged engine of a recipe, shared by every case on the same (nspec, npix, storage, placement)."""
    from mcmc_spec_amd import bands
    from mcmc_spec_amd.engine import Engine
    key = ('matrix_engine', nspec, npix, store, broadening)
    if key not in common._cache:
        c = _case(nspec)
        data, err, r = vc.synthetic_data(c, npix)
        eng = Engine(0)
        eng.stage_specs(c.specs)
        if broadening == 'in_path':
            eng.broaden_grid_window(_window(r), RESOLUTION, 'in_path')
        eng.stage_problem(data, err, c.fr, r, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=nspec,
                          bands=bands.make_bands(c.tables, *c.vega), av_table=common.av_table_exact(), tmin=c.tmin,
                          tmax=c.tmax, prior=c.prior, rad_prior=(nspec == 3), store=store)
        common._cache[key] = eng
    return common._cache[key]


def oracle(nspec, npix, broadening='staging'):
    """{mode: (values, statuses)} of the eight probes, from the oracle; once per (nspec, npix, placement)."""
    from mcmc_spec_amd import _lib
    from oracle import mft6_oracle as orc
    key = ('matrix_oracle', nspec, npix, broadening)
    if key not in common._cache:
        c = _case(nspec)
        data, err, r = vc.synthetic_data(c, npix)
        specs, kw = c.specs, {}
        if broadening == 'in_path':
            specs = orc.broaden_specs_window(c.specs, _window(r), RESOLUTION)
            kw = dict(inpath=dict(specs_raw=c.specs, w=_window(r), resolution=RESOLUTION))
        th = vc.probes(c)
        like, post, st = np.full(vc.PROBES, np.nan), np.full(vc.PROBES, np.nan), np.zeros(vc.PROBES, dtype=np.int32)
        for i, t in enumerate(th):
            post[i] = orc.logposterior(list(t), c.fr, nspec, data, err, r, specs, c.ctm, c.ptm, c.tmi, c.tma, c.tmin, c.tmax,
                                       c.matrix, common.av_prior, prior=c.prior, rad_prior=(nspec == 3), bandlib=c.bandlib, **kw)
            try:
                like[i] = orc.loglikelihood(list(t), c.fr, nspec, data, err, r, specs, c.ctm, c.ptm, c.tmi, c.tma, c.matrix,
                                            bandlib=c.bandlib, **kw)
            except ValueError:
                st[i] = _lib.W_VALUEERROR
        # six finite probes and two rejected ones as a posterior; as a likelihood seven values and one error status
        assert tuple(np.isfinite(post)) == vc.FINITE_AS_POSTERIOR and np.all(np.isneginf(post[6:]))
        assert np.all(np.isfinite(like[:7])) and list(st) == [0] * 7 + [_lib.W_VALUEERROR]
        common._cache[key] = {'LOGLIKE': (like, st), 'LOGPOST': (post, None), 'CHISQ': (-2.0 * like, st)}
    return common._cache[key]


def positions(n):
    """Which probe each of a batch's n walkers is: position j holds probe j % 8, and the last eight positions hold probes
    0..7 again whatever n -- so the probes sit at the first eight and the last eight positions, and on both sides of any
    boundary in between."""
    idx = np.arange(n) % vc.PROBES
    idx[n - vc.PROBES:] = np.arange(vc.PROBES)
    return idx


def evaluate(launch, th, ndim):
    """{mode: (values, statuses)} of one launch per mode through a *_batch_dev entry point."""
    import torch
    from mcmc_spec_amd import _lib
    dev = torch.device('cuda', 0)
    t = torch.from_numpy(np.ascontiguousarray(th)).to(dev)
    out = {}
    for mode in MODES:
        lp = torch.full((len(th),), 12345.0, dtype=torch.float64, device=dev)     # (a walker nobody wrote shows)
        st = torch.full((len(th),), -77, dtype=torch.int32, device=dev)
        launch(t.data_ptr(), lp.data_ptr(), st.data_ptr(), torch.cuda.current_stream(dev).cuda_stream, getattr(_lib, 'MODE_' + mode))
        torch.cuda.synchronize()
        out[mode] = (lp.cpu().numpy(), st.cpu().numpy())
    return out


def reference(nspec, npix, store='f64', broadening='staging'):
    """The eight probes alone through the reference instance of the staged problem: 256 threads, fused form."""
    from mcmc_spec_amd import _lib
    key = ('matrix_reference', nspec, npix, store, broadening)
    if key not in common._cache:
        eng = problem(nspec, npix, store, broadening)
        th = vc.probes(_case(nspec))
        eng.ctx.set_path(_lib.PATH_FUSED)
        ndim = th.shape[1]
        common._cache[key] = evaluate(lambda t, lp, st, s, mode: eng.ctx.logprob_batch_dev(t, len(th), ndim, lp, st, s, mode, 256), th, ndim)
        assert eng.ctx.last_form() == _lib.FORM_FUSED
        eng.ctx.set_path(_lib.PATH_AUTO)
    return common._cache[key]


def check_member(tag, got, idx, ref, orc_vals, tol, exact):
    """One problem's walkers of a launch (probe idx[j] at position j) against its reference instance and the oracle.
    Returns the largest relative deviation from the oracle."""
    worst = 0.0
    for mode in MODES:
        lp, st = got[mode]
        ref_lp, ref_st = ref[mode]
        want, want_st = orc_vals[mode]
        assert np.array_equal(st, ref_st[idx]), (tag, mode, 'statuses', st[:16], ref_st)
        if want_st is not None:
            assert np.array_equal(ref_st != 0, want_st != 0) and np.array_equal(ref_st[want_st != 0], want_st[want_st != 0]), (tag, mode)
        # every copy of a probe: the same bits
        first = np.array([lp[np.flatnonzero(idx == i)[0]] for i in range(vc.PROBES)])
        assert np.array_equal(lp, first[idx], equal_nan=True), (tag, mode, 'copies of a probe differ',
                                                                np.flatnonzero(~((lp == first[idx]) | (np.isnan(lp) & np.isnan(first[idx]))))[:8])
        fin = np.isfinite(want)
        assert np.array_equal(np.isfinite(first), fin), (tag, mode, first, want)
        assert fin.sum() >= 6
        ok = np.ones(vc.PROBES, dtype=bool) if want_st is None else want_st == 0   # (an error status carries no value)
        assert np.array_equal(np.isneginf(first[ok]), np.isneginf(want[ok])), (tag, mode)
        e = float(rel_err(first[fin], want[fin]).max())
        worst = max(worst, e)
        assert e < tol, (tag, mode, 'against the oracle', e)
        if exact:
            assert np.array_equal(first, ref_lp, equal_nan=True), (tag, mode, 'bits differ from the reference instance', first, ref_lp)
        else:
            assert np.array_equal(np.isfinite(first), np.isfinite(ref_lp)) and \
                rel_err(first[fin], ref_lp[fin]).max() < INPATH_TOL, (tag, mode, first, ref_lp)
    return worst


SINGLES = [c for c in vc.CASES if c.kind == 'single']
GROUPS = [c for c in vc.CASES if c.kind == 'group']


@pytest.mark.parametrize('case', SINGLES, ids=[c.id for c in SINGLES])
def test_instance_matches_the_oracle_and_the_reference_instance(case):
    from mcmc_spec_amd import _lib
    _no_switches()
    eng = problem(case.nspec, case.npix, case.store, case.broadening)
    ref = reference(case.nspec, case.npix, case.store, case.broadening)
    ctx = eng.ctx
    cus = ctx.device_info()['cus']
    ctx.set_path(case.path)
    try:
        # (what a launch of the most walkers a case may take would put into its first sub-batch: the form's rows, if fewer)
        rows = ctx.launch_info(vc.MAX_WALKERS_PER_CU * cus, _lib.MODE_LOGPOST, case.block)['walkers_per_sub_batch']
        n = case.walkers(cus, rows)
        assert 2 * vc.PROBES <= n <= vc.MAX_WALKERS_PER_CU * cus
        for mode in MODES:   # 1. the planner takes the instance the case names, in every mode evaluated
            info = ctx.launch_info(n, getattr(_lib, 'MODE_' + mode), case.block)
            assert info['kernel'] == case.kernel, \
                'the recipe %r (%d px, %d walkers on %d CUs, block %d) no longer reaches\n  %s\nthe planner takes\n  %s' % (
                    case.id, case.npix, n, cus, case.block, case.kernel, info['kernel'])
            assert info['form_id'] == case.form
        if case.walkers is vc.straddle and n > 3 * vc.PROBES:
            assert info['walkers_per_sub_batch'] < n <= info['walkers_per_sub_batch'] + vc.PROBES   # both sides of the boundary
        idx = positions(n)
        th = vc.probes(_case(case.nspec))[idx]
        ndim = th.shape[1]
        got = evaluate(lambda t, lp, st, s, mode: (ctx.logprob_batch_dev(t, n, ndim, lp, st, s, mode, case.block),
                                                    _assert_form(ctx, case)), th, ndim)
    finally:
        ctx.set_path(_lib.PATH_AUTO)
    tol = BASELINE_TOL if case.store == 'f32' else TIGHT
    worst = check_member(case.id, got, idx, ref, oracle(case.nspec, case.npix, case.broadening), tol, case.form != _lib.FORM_INPATH)
    print('\n%s: %d walkers x %d px ran %s\n%s: largest relative deviation from the oracle %.3e' % (
        case.id, n, case.npix, case.kernel, case.id, worst))


def _assert_form(ctx, case):
    assert ctx.last_form() == case.form, (case.id, ctx.last_form())


@pytest.mark.parametrize('case', GROUPS, ids=[c.id for c in GROUPS])
def test_group_instance_matches_the_oracle_and_the_members_reference_instances(case):
    from mcmc_spec_amd import _lib
    _no_switches()
    engines = [problem(case.nspec, npix) for npix in case.npix]
    refs = [reference(case.nspec, npix) for npix in case.npix]
    cus = engines[0].ctx.device_info()['cus']
    counts = list(case.walkers(cus, 0))
    assert min(counts) >= 2 * vc.PROBES and sum(counts) <= vc.MAX_WALKERS_PER_CU * cus
    grp = _lib.Group([e.ctx for e in engines])
    try:
        for mode in MODES:
            info = grp.launch_info(counts, getattr(_lib, 'MODE_' + mode), case.block)
            assert info['kernel'] == case.kernel, \
                'the recipe %r (%s px, %s walkers on %d CUs, block %d) no longer reaches\n  %s\nthe planner takes\n  %s' % (
                    case.id, case.npix, counts, cus, case.block, case.kernel, info['kernel'])
        idxs = [positions(n) for n in counts]
        probes = vc.probes(_case(case.nspec))
        th = np.concatenate([probes[i] for i in idxs])
        ndim = th.shape[1]
        got = evaluate(lambda t, lp, st, s, mode: grp.logprob_batch_dev(t, counts, ndim, lp, st, s, mode, case.block), th, ndim)
    finally:
        grp.close()
    worst, o = 0.0, 0
    for k, (npix, n) in enumerate(zip(case.npix, counts)):
        mine = {mode: (got[mode][0][o:o + n], got[mode][1][o:o + n]) for mode in MODES}
        worst = max(worst, check_member('%s member %d' % (case.id, k), mine, idxs[k], refs[k], oracle(case.nspec, npix), TIGHT, True))
        o += n
    print('\n%s: %s walkers x %s px ran %s\n%s: largest relative deviation from the oracle %.3e' % (
        case.id, counts, case.npix, case.kernel, case.id, worst))


def _spread(c, n, seed):
    """n walkers around the golden case's first theta: tests/test_gpu_group_chain.py's spread, fifty times tighter -- the
    synthetic spectra's posteriors are a few K wide, and a chain that accepts nothing would carry none of the kernel's values."""
    ns = c.nspec
    sc = np.array([30.0] * ns + [0.02] + [0.02] * ns + [2e-5]) * 0.02
    th = c.theta[0] + np.random.default_rng(seed).normal(size=(n, 2 * ns + 2)) * sc
    th[:, :ns] = np.clip(th[:, :ns], c.tmin + 0.1, c.tmax - 0.1)   # (the triple's tertiary sits 1 K above the box's edge)
    return th


@pytest.mark.parametrize('case', vc.SAMPLER_CASES, ids=[s.id for s in vc.SAMPLER_CASES])
def test_group_sampler_instance_walks_the_host_chain(case):
    """msx_group_sampler_begin plans the members' half-counts (Group.launch_info says which entry) and launches that
    entry's SMP twin, or -- for an entry built without one -- its neighbour without PF, then without SH (case.runs):
    three iterations on the device, bit for bit the chain of GroupSampler, the host definition."""
    from mcmc_spec_amd.group import DeviceGroupSampler, GroupSampler, TargetGroup
    _no_switches()
    c = _case(case.nspec)
    engines = [problem(case.nspec, npix) for npix in case.npix]
    cus = engines[0].ctx.device_info()['cus']
    half = list(case.half_counts(cus))
    counts = [2 * h for h in half]
    assert sum(counts) <= vc.MAX_WALKERS_PER_CU * cus
    grp = TargetGroup(engines)
    try:
        info = grp.launch_info(half)
        assert info['kernel'] == case.planned, \
            'the sampler recipe %r (%s px, half-counts %s on %d CUs) no longer plans\n  %s\nbut\n  %s' % (
                case.id, case.npix, half, cus, case.planned, info['kernel'])
        ndim, n, seeds = 2 * case.nspec + 2, 3, [11, 12]
        p0s = [_spread(c, counts[k], 900 + k) for k in range(2)]
        dev = DeviceGroupSampler(counts, ndim, grp, seeds=seeds, chunk=2)
        dev.run_mcmc(p0s, n)
        host = GroupSampler(counts, ndim, grp.logposterior, seeds=seeds)
        host.run_mcmc(p0s, n)
        for k in range(2):
            assert dev.get_chain(k).shape == (n, counts[k], ndim)
            assert np.array_equal(dev.get_chain(k), host.get_chain(k)), (case.id, k)
            assert np.array_equal(dev.get_log_prob(k), host.get_log_prob(k)), (case.id, k)
            assert np.array_equal(dev.acceptance_fraction[k], host.acceptance_fraction[k]), (case.id, k)
            assert np.isfinite(dev.get_log_prob(k)).all()
        assert sum(float(a.sum()) for a in dev.acceptance_fraction) > 0.0   # the chain moved: the kernel's values are in it
    finally:
        grp.close()
    print('\n%s: half-counts %s x %s px planned %s, ran the SMP instance <%s>' % (case.id, half, case.npix, case.planned, case.runs))
