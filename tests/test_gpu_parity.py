"""GPU parity tests proper: the HIP path (through the C ABI) against the reference-generated golden
vectors and against the CPU oracle on identical inputs.  Tolerance on log-probabilities is the
north-star's 1e-6 relative; what is actually observed is ~1e-12, and the tighter bound 1e-9 is
asserted so regressions in summation order or table staging are caught early."""
import os

import numpy as np
import pytest

import common
from common import golden_case, oracle_loglike, oracle_logpost, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-6      # north-star bar
TIGHT = 1e-9    # what float64 with re-ordered sums should easily meet


def make_engine(c, rad_prior=False, with_prior=True):
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd import bands
    eng = Engine(0)
    eng.stage_specs(c.specs)
    bl = bands.make_bands(c.tables, *c.vega)
    eng.stage_problem(c.data, c.err, c.fr, c.r, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=c.nspec, bands=bl,
                      av_table=common.av_table_exact() if with_prior else None, tmin=c.tmin, tmax=c.tmax,
                      prior=c.prior if with_prior else 0, rad_prior=rad_prior)
    return eng


@pytest.fixture(scope='module')
def engA():
    return make_engine(golden_case('A'))


@pytest.fixture(scope='module')
def engB():
    return make_engine(golden_case('B'))


@pytest.mark.parametrize('which', ['A', 'B'])
def test_loglikelihood_matches_reference_golden(which, engA, engB):
    c = golden_case(which)
    eng = engA if which == 'A' else engB
    got = eng.loglikelihood(c.theta)
    want = c.g[which + '_loglike']
    e = rel_err(got, want)
    print('case', which, 'max rel err vs reference', e.max())
    assert e.max() < TIGHT
    # walker-at-a-time entry returns a Python float like the reference
    one = eng.loglikelihood(c.theta[0])
    assert isinstance(one, float) and one == got[0]


def test_chisq_mode_matches(engB):
    c = golden_case('B')
    got = engB.loglikelihood(c.theta, optimize=True)
    assert rel_err(got, -2.0 * c.g['B_loglike']).max() < TIGHT


@pytest.mark.parametrize('rad_prior', [False, True])
def test_logposterior_matches_reference_golden(rad_prior):
    c = golden_case('A')
    eng = make_engine(c, rad_prior=rad_prior)
    th = c.g['theta_post']
    got = eng.logposterior(th)
    want = c.g['A_logpost_' + ('radprior' if rad_prior else 'noradprior')]
    assert np.array_equal(np.isinf(got), np.isinf(want))
    assert rel_err(got, want).max() < TIGHT


def test_vs_oracle_random_walkers(engB):
    c = golden_case('B')
    rng = np.random.default_rng(99)
    th = c.theta[0] + rng.normal(size=(64, 6)) * np.array([120, 120, 0.05, 0.05, 0.05, 1e-4])
    th[:, 0:2] = np.clip(th[:, 0:2], 3000.0, 4200.0)
    th[:, 2] = np.abs(th[:, 2])
    th[:, 3:5] = np.clip(th[:, 3:5], 0.05, 1.4)
    got = engB.loglikelihood(th)
    want = np.array([oracle_loglike(c, t) for t in th])
    assert rel_err(got, want).max() < TIGHT


def test_run_to_run_bitwise_deterministic(engB):
    c = golden_case('B')
    a = engB.logposterior(c.theta)
    b = engB.logposterior(c.theta)
    assert np.array_equal(a, b)
    # batch composition must not matter either: same walkers in another order / batch size
    perm = np.random.default_rng(1).permutation(len(c.theta))
    d = engB.logposterior(c.theta[perm])
    assert np.array_equal(d, a[perm])


def test_make_composite_matches_reference_golden(engB):
    from oracle import mft6_oracle as orc
    c = golden_case('B')
    p = c.theta[0]
    lg = [float(orc.get_logg(t, c.matrix)) for t in p[:2]]
    wl, spec, con, pcw, ph = engB.make_composite(p[:2], lg, p[3:5], p[5])
    g = c.g
    assert wl[0] == g['B_mc_wl_ends'][0] and wl[-1] == g['B_mc_wl_ends'][1] and len(wl) == g['B_mc_wl_ends'][2]
    assert rel_err(spec[::211], g['B_mc_spec_sub']).max() < 1e-13
    assert rel_err(con, g['B_mc_contrast']).max() < 1e-11
    assert rel_err(ph, g['B_mc_phot']).max() < 1e-11


def test_error_conventions():
    c = golden_case('B')
    eng = make_engine(c)
    # Teff outside the isochrone table -> interp1d ValueError in the reference (mft6.py:95)
    bad = c.theta[0].copy()
    bad[1] = 2800.0
    with pytest.raises(ValueError):
        eng.loglikelihood(bad)
    # ... but the posterior rejects it in the prior box first (mft6.py:1227) -> -inf, no exception
    assert eng.logposterior(bad) == -np.inf
    # two different failures on the two stars: every star's logg is interpolated before the first star's spectrum is
    # built (mft6.py:1149), so the secondary's ValueError wins over the primary's IndexError (beyond the last node)
    both = c.theta[0].copy()
    both[0], both[1] = 4325.0, 2874.0
    from oracle import mft6_oracle as orc
    with pytest.raises(ValueError):
        orc.loglikelihood(list(both), c.fr, 2, c.data, c.err, c.r, c.specs, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, bandlib=c.bandlib)
    with pytest.raises(ValueError):
        eng.loglikelihood(both)
    both[1] = 3500.0
    with pytest.raises(IndexError):
        eng.loglikelihood(both)
    # wrong length
    with pytest.raises(ValueError):
        eng.loglikelihood(np.zeros(5))
    # missing node -> KeyError (mft6.py:489-500)
    specs = dict(c.specs)
    del specs['3800, 5.0']
    from mcmc_spec_amd.engine import Engine
    e2 = Engine(0)
    e2.stage_specs(specs)
    e2.stage_problem(c.data, c.err, c.fr, c.r, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=2,
                     bands=__import__('mcmc_spec_amd.bands', fromlist=['x']).make_bands(c.tables, *c.vega))
    with pytest.raises(KeyError):
        e2.loglikelihood(c.theta[0])
    # non-finite coordinates never produce NaN
    nf = c.theta[0].copy()
    nf[2] = np.nan
    assert eng.logposterior(nf) == -np.inf


def test_broaden_and_ccm89_vs_oracle():
    from oracle import mft6_oracle as orc
    from mcmc_spec_amd._lib import Context
    ctx = Context(0)
    wl = np.arange(6450.0, 8400.0, 0.2)
    rng = np.random.default_rng(5)
    f = 1.0 + 0.3 * np.sin(wl / 7.0) + 0.05 * rng.normal(size=len(wl))
    for R in (1700, 5000, 400):
        got = ctx.broaden(wl, f, R)
        _, want = orc.broaden(wl, f, R)
        assert rel_err(got, want).max() < 1e-12, R
    w = np.concatenate([np.linspace(3050, 30000, 4001), [1e4 / 1.1, 1e4 / 3.3]])
    k = ctx.ccm89_k(w, 3.1)
    assert rel_err(k, orc.ccm89(w, 1.0, 3.1)).max() < 1e-13


def test_median_edge_cases():
    """Odd pixel counts, tiny spectra and heavy duplication exercise every branch of the select."""
    c = golden_case('B')
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd import bands
    bl = bands.make_bands(c.tables, *c.vega)
    eng = Engine(0)
    eng.stage_specs(c.specs)
    for npix in (699, 64, 5):
        sel = np.arange(npix)
        data = [c.data[0][sel], c.data[1][sel]]
        err = c.err[sel]
        r = [min(data[0]), max(data[0])]
        eng.stage_problem(data, err, c.fr, r, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=2, bands=bl)
        got = eng.loglikelihood(c.theta[:8])
        from oracle import mft6_oracle as orc
        want = np.array([orc.loglikelihood(list(t), c.fr, 2, data, err, r, c.specs, c.ctm, c.ptm, c.tmi, c.tma,
                                           c.matrix, bandlib=c.bandlib) for t in c.theta[:8]])
        assert rel_err(got, want).max() < TIGHT, npix


def test_median_radix_fallback_on_heavily_duplicated_values():
    """A step-function grid with A_V = 0 gives thousands of bit-identical model values, so the
    1024-bin stage finds > 256 candidates and the kernel must take the bitwise radix-select path."""
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd import synth
    from oracle import mft6_oracle as orc
    teffs = np.arange(3000, 3500, 100)
    loggs = np.array([4.5, 5.0, 5.5])
    wl = np.arange(5400, 9100, 0.2)
    flux = np.empty((len(teffs), len(loggs), len(wl)))
    for i, t in enumerate(teffs):
        for j, g in enumerate(loggs):
            flux[i, j] = np.where(wl < 7000.0, 1.0e5, 3.0e5) * (1 + 0.01 * i + 0.02 * j) \
                + np.where((wl > 7500) & (wl < 7600), 1.0e5 * np.sin(wl), 0.0)
    specs = synth.grid_to_specs(teffs, loggs, wl, flux)
    matrix = synth.make_isochrone_matrix()
    ctm = [[list(np.linspace(6000, 8800, 40))], [list(np.ones(40))], [0], [7400.0]]
    ptm = [[], [], [], []]
    fr = [[1.0], [0.1], ['x'], [], [], []]
    for npix in (2048, 2047):
        wl_um = np.linspace(0.56, 0.88, npix)
        rng = np.random.default_rng(4)
        data = [wl_um, 1 + 0.05 * rng.normal(size=npix)]
        err = np.full(npix, 0.05)
        r = [wl_um.min(), wl_um.max()]
        eng = Engine(0)
        eng.stage_specs(specs)
        eng.stage_problem(data, err, fr, r, ctm, ptm, 6000.0, 8800.0, matrix, nspec=2)
        th = np.array([[3250.0, 3120.0, 0.0, 0.5, 0.4, 2e-3], [3300.0, 3049.0, 0.0, 0.7, 0.9, 3e-3],
                       [3250.0, 3120.0, 0.3, 0.5, 0.4, 2e-3]])
        got = eng.loglikelihood(th)
        want = np.array([orc.loglikelihood(list(t), fr, 2, data, err, r, specs, ctm, ptm, 6000.0, 8800.0, matrix)
                         for t in th])
        assert rel_err(got, want).max() < TIGHT, npix


@pytest.mark.parametrize('shape', ['two_clusters', 'wide_range', 'plateau_at_median', 'flat'])
def test_early_histogram_median_branches(shape):
    """The median whose histogram is filled during phase A (logbin_median) and its exits: the upper middle value
    in a LATER bin than the lower one (two clusters, even count), a vector spanning more than 8 binades (falls
    back to the min/max-binned select), 65..256 equal candidates in the median's bin (ranked through LDS), and a
    constant vector (min == max).  All against the oracle, even and odd pixel counts."""
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd import synth
    from oracle import mft6_oracle as orc
    teffs = np.arange(3000, 3500, 100)
    loggs = np.array([4.5, 5.0, 5.5])
    wl = np.arange(5400, 9100, 0.2)
    x = (wl - 5600.0) / (8800.0 - 5600.0)          # 0..1 across the data window
    if shape == 'two_clusters':
        base = np.where(x < 0.5, 1.0e5 * (1 + 1e-3 * x), 2.0e5 * (1 + 1e-3 * x))
    elif shape == 'wide_range':
        base = 1.0e5 * 10.0 ** (4.0 * np.clip(x, 0, 1))
    elif shape == 'plateau_at_median':
        base = 1.0e5 * (1 + 0.5 * np.where(np.abs(x - 0.5) < 0.035, 0.5, x))   # ~7 % of the pixels share one value
    else:
        base = np.full_like(wl, 1.0e5)
    flux = np.empty((len(teffs), len(loggs), len(wl)))
    for i in range(len(teffs)):
        for j in range(len(loggs)):
            flux[i, j] = base * (1 + 0.01 * i + 0.02 * j)
    specs = synth.grid_to_specs(teffs, loggs, wl, flux)
    matrix = synth.make_isochrone_matrix()
    ctm = [[list(np.linspace(6000, 8800, 40))], [list(np.ones(40))], [0], [7400.0]]
    ptm = [[], [], [], []]
    fr = [[1.0], [0.1], ['x'], [], [], []]
    for npix in (2048, 2047, 300):
        wl_um = np.linspace(0.56, 0.88, npix)
        rng = np.random.default_rng(4)
        data = [wl_um, 1 + 0.05 * rng.normal(size=npix)]
        err = np.full(npix, 0.05)
        r = [wl_um.min(), wl_um.max()]
        eng = Engine(0)
        eng.stage_specs(specs)
        eng.stage_problem(data, err, fr, r, ctm, ptm, 6000.0, 8800.0, matrix, nspec=2)
        th = np.array([[3250.0, 3120.0, 0.0, 0.5, 0.4, 2e-3], [3300.0, 3049.0, 0.0, 0.7, 0.9, 3e-3],
                       [3250.0, 3120.0, 0.3, 0.5, 0.4, 2e-3]])
        want = np.array([orc.loglikelihood(list(t), fr, 2, data, err, r, specs, ctm, ptm, 6000.0, 8800.0, matrix)
                         for t in th])
        import torch
        from mcmc_spec_amd import _lib
        dev = torch.device('cuda', 0)
        tht = torch.from_numpy(np.ascontiguousarray(th)).to(dev)
        for block in (0, 256, _lib.BLOCK_512_SHARED):   # auto = 512 threads with LDS-staged statics; the others without
            lp = torch.empty(len(th), dtype=torch.float64, device=dev)
            st = torch.empty(len(th), dtype=torch.int32, device=dev)
            eng.ctx.logprob_batch_dev(tht.data_ptr(), len(th), 6, lp.data_ptr(), st.data_ptr(),
                                      torch.cuda.current_stream(dev).cuda_stream, _lib.MODE_LOGLIKE, block)
            torch.cuda.synchronize()
            assert int(st.abs().sum()) == 0
            assert rel_err(lp.cpu().numpy(), want).max() < TIGHT, (shape, npix, block)


@pytest.mark.parametrize('block', [256, 512, 1512])   # 1512 = MSX_BLOCK_512_SHARED
def test_every_workgroup_size_gives_identical_bits(block, engB):
    import torch
    from mcmc_spec_amd import _lib
    c = golden_case('B')
    ref = engB.loglikelihood(c.theta)
    dev = torch.device('cuda', 0)
    th = torch.from_numpy(np.ascontiguousarray(c.theta)).to(dev)
    lp = torch.empty(len(c.theta), dtype=torch.float64, device=dev)
    st = torch.empty(len(c.theta), dtype=torch.int32, device=dev)
    engB.ctx.logprob_batch_dev(th.data_ptr(), len(c.theta), 6, lp.data_ptr(), st.data_ptr(),
                               torch.cuda.current_stream(dev).cuda_stream, _lib.MODE_LOGLIKE, block)
    torch.cuda.synchronize()
    assert rel_err(lp.cpu().numpy(), c.g['B_loglike']).max() < TIGHT
    assert int(st.abs().sum()) == 0
    del ref


def test_bits_do_not_depend_on_workgroup_size_or_batch():
    """the gathered vector of a sharded run must be bit-identical to the one-GPU vector.  Shards are
    launched with other batch sizes, hence other workgroup sizes, so every sum of the kernel is taken in an order
    that is independent of both (1024 accumulator slots, 16 virtual waves).  Weak contrast terms here, so that the spectral chi^2 -- the
    part that is summed over pixels -- carries the value's low bits."""
    import torch
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd import bands
    c = golden_case('B')
    bl = bands.make_bands(c.tables, *c.vega)
    fr = [list(c.fr[0]), [10.0 for _ in c.fr[1]], c.fr[2], list(c.fr[3]), [10.0 for _ in c.fr[4]], c.fr[5]]
    eng = Engine(0)
    eng.stage_specs(c.specs)
    eng.stage_problem(c.data, c.err, fr, [min(c.data[0]), max(c.data[0])], c.ctm, c.ptm, c.tmi, c.tma, c.matrix,
                      nspec=2, bands=bl)
    rng = np.random.default_rng(8)
    th = np.repeat(c.theta[:8], 40, axis=0) * (1 + 1e-3 * rng.normal(size=(320, 6)))
    dev = torch.device('cuda', 0)
    tht = torch.from_numpy(np.ascontiguousarray(th)).to(dev)
    out = {}
    for mode in (_lib.MODE_LOGLIKE, _lib.MODE_CHISQ):
        for block in (256, 512, _lib.BLOCK_512_SHARED, 0):
            lp = torch.empty(len(th), dtype=torch.float64, device=dev)
            st = torch.empty(len(th), dtype=torch.int32, device=dev)
            eng.ctx.logprob_batch_dev(tht.data_ptr(), len(th), 6, lp.data_ptr(), st.data_ptr(),
                                      torch.cuda.current_stream(dev).cuda_stream, mode, block)
            torch.cuda.synchronize()
            out[mode, block] = lp.cpu().numpy()
        ref = out[mode, 256]
        assert np.isfinite(ref).sum() > 100
        for block in (512, _lib.BLOCK_512_SHARED, 0):
            assert np.array_equal(out[mode, block], ref, equal_nan=True), (mode, block)
        # a shard of the batch (other n -> other automatic workgroup size, 512 threads with LDS-staged statics)
        lp = torch.empty(100, dtype=torch.float64, device=dev)
        st = torch.empty(100, dtype=torch.int32, device=dev)
        eng.ctx.logprob_batch_dev(tht[57:157].contiguous().data_ptr(), 100, 6, lp.data_ptr(), st.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream, mode, 0)
        torch.cuda.synchronize()
        assert np.array_equal(lp.cpu().numpy(), ref[57:157], equal_nan=True)


def test_generic_recipe_path_for_large_tables():
    """Tables too large for the register-resident recipe (here a 300-bin A_V table) take the generic
    memory-walking path; results must not change."""
    from oracle import mft6_oracle as orc
    c = golden_case('B')
    edges = np.linspace(4.0, 3000.0, 301)
    mu = 0.05 + 0.0007 * np.arange(300)
    sig = np.where(np.arange(300) % 7 == 0, 0.0, 0.04)  # sigma == 0 -> 0.05 (mft6.py:1237)

    def avp(d):
        b = int(np.clip(np.searchsorted(edges, d, side='right') - 1, 0, 299))
        return mu[b], sig[b]

    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd import bands
    eng = Engine(0)
    eng.stage_specs(c.specs)
    eng.stage_problem(c.data, c.err, c.fr, c.r, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=2,
                      bands=bands.make_bands(c.tables, *c.vega), av_table=(edges, mu, sig), tmin=c.tmin, tmax=c.tmax,
                      prior=c.prior, rad_prior=True)
    got = eng.logposterior(c.g['theta_post'])
    want = np.array([orc.logposterior(list(t), c.fr, 2, c.data, c.err, c.r, c.specs, c.ctm, c.ptm, c.tmi, c.tma,
                                      c.tmin, c.tmax, c.matrix, avp, prior=c.prior, rad_prior=True,
                                      bandlib=c.bandlib) for t in c.g['theta_post']])
    assert np.array_equal(np.isinf(got), np.isinf(want))
    assert rel_err(got, want).max() < TIGHT


# ------------------------------------------------------------------------------------------------
# the drop-in module: reference signatures, identity cache, sampler protocol (config 1 plumbing)
# ------------------------------------------------------------------------------------------------
def _dropin(c):
    import mcmc_spec_amd.mft6 as m
    from mcmc_spec_amd import bands
    m.clear_cache()
    m.set_band_library(bands.make_bands(c.tables, *c.vega))
    m.set_av_prior(*common.av_table_exact())
    return m


def test_dropin_signatures_match_reference_golden():
    c = golden_case('A')
    m = _dropin(c)
    args = [c.fr, 2, 0, c.data, c.err, 1700, c.r, c.specs, c.ctm, c.ptm, c.tmi, c.tma, None]
    th = c.g['theta_post']
    # logposterior(p0, fr, nspec, ndust, data, err, broadening, r, specs, ctm, ptm, tmi, tma, vs, tmin, tmax,
    #              matrix, ra, dec, **kwargs) -- positional exactly like mft6.py:1491-1492
    post_args = args + [c.tmin, c.tmax, c.matrix, 10.0, 20.0]
    kw = dict(dust=False, norm=True, prior=c.prior, a=True, models='btsettl', dist_fit=True, rad_prior=True)
    got = m.logposterior(th, *post_args, **kw)
    want = c.g['A_logpost_radprior']
    assert np.array_equal(np.isinf(got), np.isinf(want)) and rel_err(got, want).max() < TIGHT
    one = m.logposterior(list(th[0]), *post_args, **kw)
    assert isinstance(one, float) and one == got[0]
    ll = m.loglikelihood(c.theta, *(args + [c.matrix]))
    assert rel_err(ll, c.g['A_loglike']).max() < TIGHT
    chi = m.loglikelihood(c.theta[0], *(args + [c.matrix]), optimize=True)
    assert abs(chi + 2 * c.g['A_loglike'][0]) < 1e-9 * abs(chi)
    lp = m.logprior(th, 2, 0, c.tmin, c.tmax, c.matrix, 10.0, 20.0, prior=c.prior, ext=True, dist_fit=True,
                    rad_prior=True)
    wantp = c.g['A_logprior_radprior']
    assert np.array_equal(np.isinf(lp), np.isinf(wantp)) and rel_err(lp, wantp).max() < 1e-12
    with pytest.raises(ValueError):
        m.logposterior(np.zeros(7), *post_args, **kw)


def test_dropin_device_sampler_walks_the_chain_of_the_emcee_line():
    """run_emcee's sampler line (mft6.py:1490-1492) with the same args / kwargs: the host sampler over the drop-in
    logposterior and mft6.device_sampler give one chain, bit for bit; argument mistakes fail like the function's."""
    from mcmc_spec_amd.sampler import EnsembleSampler
    c = golden_case('A')
    m = _dropin(c)
    args = [c.fr, 2, 0, c.data, c.err, 1700, c.r, c.specs, c.ctm, c.ptm, c.tmi, c.tma, None, c.tmin, c.tmax, c.matrix,
            10.0, 20.0]
    kw = dict(dust=False, norm=True, prior=c.prior, a=True, models='btsettl', dist_fit=True, rad_prior=True)
    rng = np.random.default_rng(3)
    p0 = c.theta[0] + rng.normal(size=(32, 6)) * np.array([20, 20, 0.02, 0.02, 0.02, 2e-5])
    host = EnsembleSampler(32, 6, m.logposterior, args=args, kwargs=kw, vectorize=True, seed=4)
    hs = host.run_mcmc(p0, 30)
    dev = m.device_sampler(32, 6, args=args, kwargs=kw, seed=4, chunk=8)
    ds = dev.run_mcmc(p0, 30)
    assert np.array_equal(dev.get_chain(), host.get_chain()) and np.array_equal(dev.get_log_prob(), host.get_log_prob())
    assert np.array_equal(ds.coords, hs.coords) and 0.05 < dev.acceptance_fraction.mean() < 0.95
    with pytest.raises(TypeError):
        m.device_sampler(32, 6, args=args, kwargs=dict(kw, bogus=1))
    with pytest.raises(TypeError):
        m.device_sampler(32, 6, args=args[:-3], kwargs=kw)
    with pytest.raises(ValueError):
        m.device_sampler(32, 8, args=args, kwargs=kw)


def test_dropin_logprior_with_two_live_datasets():
    """logprior takes its dataset from the LAST staging call (or from `specs=`), explicitly -- and since the value
    depends on p0 and the prior arguments only, it is the same whichever dataset carries it."""
    import mcmc_spec_amd.mft6 as m
    from mcmc_spec_amd import bands
    a, b = golden_case('A'), golden_case('B')
    m.clear_cache()
    m.set_band_library(bands.make_bands(b.tables, *b.vega))
    m.set_av_prior(*common.av_table_exact())
    th = a.g['theta_post']
    with pytest.raises(RuntimeError):
        m.logprior(th, 2, 0, a.tmin, a.tmax, a.matrix, 10.0, 20.0, prior=a.prior)
    m.loglikelihood(th[:4], a.fr, 2, 0, a.data, a.err, 1700, a.r, a.specs, a.ctm, a.ptm, a.tmi, a.tma, None, a.matrix)
    lp_a = m.logprior(th, 2, 0, a.tmin, a.tmax, a.matrix, 10.0, 20.0, prior=a.prior, rad_prior=True)
    specs_b = dict(b.specs)     # a second grid object + dataset alive at the same time
    m.loglikelihood(th[:4], b.fr, 2, 0, b.data, b.err, 1700, b.r, specs_b, b.ctm, b.ptm, b.tmi, b.tma, None, b.matrix)
    lp_b = m.logprior(th, 2, 0, a.tmin, a.tmax, a.matrix, 10.0, 20.0, prior=a.prior, rad_prior=True)
    lp_a2 = m.logprior(th, 2, 0, a.tmin, a.tmax, a.matrix, 10.0, 20.0, prior=a.prior, rad_prior=True, specs=a.specs)
    assert np.array_equal(lp_a, lp_b) and np.array_equal(lp_a, lp_a2)
    assert rel_err(lp_a, a.g['A_logprior_radprior']).max() < 1e-12
    with pytest.raises(RuntimeError):
        m.logprior(th, 2, 0, a.tmin, a.tmax, a.matrix, 10.0, 20.0, prior=a.prior, specs=dict(a.specs))
    m.clear_cache()


def test_dropin_make_composite_and_broaden():
    from oracle import mft6_oracle as orc
    c = golden_case('B')
    m = _dropin(c)
    p = c.theta[0]
    lg = [float(orc.get_logg(t, c.matrix)) for t in p[:2]]
    wl, spec, con, pcw, ph = m.make_composite(p[:2], lg, p[3:5], p[5], c.fr[2], c.fr[5], c.r, c.specs, c.ctm, c.ptm,
                                              c.tmi, c.tma, None, nspec=2)
    assert len(wl) == c.g['B_mc_wl_ends'][2] and rel_err(spec[::211], c.g['B_mc_spec_sub']).max() < 1e-13
    assert rel_err(con, c.g['B_mc_contrast']).max() < 1e-11 and rel_err(ph, c.g['B_mc_phot']).max() < 1e-11
    assert np.allclose(pcw, [np.mean(w) for w in c.ptm[0]])
    # distance=False branch (mft6.py:701-703): secondary scaled by rad[0]^2 only
    w2, s2, con2, _, _ = m.make_composite(p[:2], lg, p[3:5], False, c.fr[2], c.fr[5], c.r, c.specs, c.ctm, c.ptm,
                                          c.tmi, c.tma, None, nspec=2)
    wo, so, cono, _, _, _ = orc.make_composite(p[:2], lg, p[3:5], False, c.fr[2], c.fr[5], c.r, c.specs, c.ctm, c.ptm,
                                               c.tmi, c.tma, bandlib=c.bandlib)
    assert rel_err(s2, so).max() < 1e-13 and rel_err(con2, cono).max() < 1e-11
    wl_b = np.arange(6450.0, 8400.0, 0.2)
    f = 1 + 0.2 * np.cos(wl_b / 3.0)
    ww, bb = m.broaden(wl_b, f, 1700)
    assert rel_err(bb, orc.broaden(wl_b, f, 1700)[1]).max() < 1e-12


def test_config1_plumbing_sampler_over_the_gpu_logposterior():
    """BASELINE config 1 shape: binary fit on Data/synth_spec_3850_3025.txt (golden dataset A), 32 walkers,
    emcee protocol with vectorize=True -> one fused launch per half-ensemble.  Pass = chain runs, every
    log-prob finite and equal to the oracle's at the final state."""
    from mcmc_spec_amd.sampler import EnsembleSampler
    c = golden_case('A')
    m = _dropin(c)
    args = [c.fr, 2, 0, c.data, c.err, 1700, c.r, c.specs, c.ctm, c.ptm, c.tmi, c.tma, None, c.tmin, c.tmax, c.matrix,
            10.0, 20.0]
    kw = dict(prior=c.prior, a=True, dist_fit=True, rad_prior=False)
    s = EnsembleSampler(32, 6, m.logposterior, args=args, kwargs=kw, vectorize=True, seed=1)
    rng = np.random.default_rng(1)
    p0 = c.theta[0] + rng.normal(size=(32, 6)) * np.array([20, 20, 0.01, 0.01, 0.01, 1e-5])
    st = s.run_mcmc(p0, 100)
    assert s.chain.shape == (32, 100, 6) and np.all(np.isfinite(st.log_prob))
    want = np.array([oracle_logpost(c, t) for t in st.coords[:6]])
    assert rel_err(st.log_prob[:6], want).max() < TOL
    assert s.acceptance_fraction.mean() > 0.02


def test_triple_system_ndim8_matches_reference_golden():
    """nspec = 3 (ndim 8): three components, contrast list split secondary/tertiary (mft6.py:746-751),
    triple prior box (mft6.py:1347) with rad_prior=True (the only ndim-8 prior path that returns a value)."""
    c = golden_case('C')
    eng = make_engine(c, rad_prior=True)
    g = c.g
    got = eng.logposterior(c.theta)
    want = g['C_logpost']
    assert np.array_equal(np.isinf(got), np.isinf(want)) and rel_err(got, want).max() < TIGHT
    ok = np.isfinite(g['C_loglike'])
    ll = eng.loglikelihood(c.theta[ok])
    assert rel_err(ll, g['C_loglike'][ok]).max() < TIGHT
    lp = eng.logprior(c.theta)
    assert np.array_equal(np.isinf(lp), np.isinf(g['C_logprior'])) and rel_err(lp, g['C_logprior']).max() < 1e-12
    # the triple-system kernel variants (256 / 512 threads, alone or sharing a CU) agree to the bit
    import torch
    from mcmc_spec_amd import _lib
    dev = torch.device('cuda', 0)
    tht = torch.from_numpy(np.ascontiguousarray(c.theta)).to(dev)
    for block in (256, 512, _lib.BLOCK_512_SHARED):
        out = torch.empty(len(c.theta), dtype=torch.float64, device=dev)
        st = torch.empty(len(c.theta), dtype=torch.int32, device=dev)
        eng.ctx.logprob_batch_dev(tht.data_ptr(), len(c.theta), 8, out.data_ptr(), st.data_ptr(),
                                  torch.cuda.current_stream(dev).cuda_stream, _lib.MODE_LOGPOST, block)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), got, equal_nan=True), block


def test_loader_spec_interpolator_matches_reference_golden(tmp_path):
    """f3: text files -> resample -> stage -> broaden on the device, against the reference's own
    spec_interpolator output (golden) on the same synthetic BT-Settl-format files."""
    from mcmc_spec_amd import loader, synth
    import mcmc_spec_amd.mft6 as m
    g = golden_case('A').g
    gdir = synth.write_btsettl_text_grid(str(tmp_path / 'BT-Settl_M-0.0a+0.0'), seed=21)
    m.clear_cache()
    specs = loader.spec_interpolator([6000.0, 8000.0], [3000, 3200], [4, 5.5], [5000, 9000], resolution=1700,
                                     grid_dir=gdir, cache=str(tmp_path / 'grid_cache.npz'))
    keys = sorted(k for k in specs if k != 'wl')
    assert keys == list(g['L_keys'])
    assert [specs['wl'][0], specs['wl'][-1], len(specs['wl'])] == list(g['L_wl_ends'])
    for k, want in zip(keys, g['L_sub']):
        assert rel_err(specs[k][::53], want).max() < 1e-12, k
    # second call is served from the binary cache and stages the same bits
    again = loader.spec_interpolator([6000.0, 8000.0], [3000, 3200], [4, 5.5], [5000, 9000], resolution=1700,
                                     grid_dir=gdir, cache=str(tmp_path / 'grid_cache.npz'))
    assert all(np.array_equal(again[k], specs[k]) for k in specs)
    assert m._engine_for(specs) is specs.engine  # the drop-in API reuses the staged grid
    with pytest.raises(ValueError):  # resample range check = interp1d's ValueError
        specs.engine.ctx.resample_linear(np.array([1.0, 2.0, 3.0]), np.ones(3), np.array([0.5]))


def test_fit_spec_trajectory_matches_the_reference(tmp_path):
    """f4: the reference's fit_spec was run with its proposal draws redirected to a seeded Generator
    (tests/golden/make_golden.py); the batched GPU optimiser with the same seed must walk the same
    trajectory: same accepted parameters, same running-best chi^2, same test chi^2 per proposal."""
    from mcmc_spec_amd import bands, optimizer
    from mcmc_spec_amd.engine import Engine
    c = golden_case('B')
    g = c.g
    eng = Engine(0)
    eng.stage_specs(c.specs)
    eng.stage_problem(c.data, c.err, c.fr, c.r, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=2,
                      bands=bands.make_bands(c.tables, *c.vega))
    # initial-guess kernel vs the oracle's restatement
    from oracle import mft6_oracle as orc
    st = g['D_start']
    like0, _ = eng.ctx.opt_init(st[None, :])
    assert rel_err(like0[0], g['D_init_like'][0]) < TIGHT
    res = optimizer.fit_spec_batch(eng, st[None, :], [3000.0, 4200.0], (2.0732e-3, 0.0277e-3), c.matrix,
                                   common.av_table_exact(), nspec=2, steps=int(g['D_steps'][0]), dist_fit=True,
                                   rad_prior=True, rngs=[np.random.default_rng(123)], dirname=str(tmp_path))
    line, best_chi, ch = res[0]
    ref = g['D_chisq']
    assert len(ch.savechi) - 1 == len(ref)
    assert rel_err(np.array(ch.savechi[1:]), ref[:, 0]).max() < TIGHT          # running best after each proposal
    # the reference's file pairs savechi[n] with savetest[n] whose first four entries are guesses, not chi^2
    assert rel_err(np.array(ch.savetest[:len(ref) - 3]), ref[3:, 1]).max() < TIGHT
    assert rel_err(best_chi, g['D_best_chi'][0]) < TIGHT
    assert rel_err(np.array([float(x) for x in line.split()]), g['D_best']).max() < 1e-12
    got_params = np.loadtxt(tmp_path / 'params0.txt')
    assert got_params.shape == g['D_params'].shape and rel_err(got_params, g['D_params']).max() < 1e-12
    # a proposal chi^2 straight against the oracle restatement of mft6.py:997-1028
    _, flux_n = orc.fit_spec_init(c.data[0] * 1e4, c.data[1], c.err, c.r, st[:2], st[3:5], st[5], c.fr, c.specs, c.ctm,
                                  c.ptm, c.tmi, c.tma, c.matrix, bandlib=c.bandlib)
    th = c.theta[:6]
    got, _ = eng.ctx.opt_step(th, np.zeros(len(th), dtype=np.int32))
    want = np.array([orc.fit_spec_proposal(c.data[0] * 1e4, flux_n, c.err, c.r, t[:2], t[2], t[3:5], t[5], c.fr, c.specs,
                                           c.ctm, c.ptm, c.tmi, c.tma, c.matrix, bandlib=c.bandlib) for t in th])
    assert rel_err(got, want).max() < TIGHT


def test_optimize_fit_batched_descends_and_writes_reference_files(tmp_path):
    from mcmc_spec_amd import optimizer
    c = golden_case('B')
    m = _dropin(c)
    out = optimizer.optimize_fit(str(tmp_path), c.data, c.err, c.specs, 24, c.fr, [2.0732e-3, 0.0277e-3], [0.106, 0.01],
                                 1700, c.ctm, c.ptm, c.tmi, c.tma, None, c.matrix, 10.0, 20.0, nspec=2, nstep=30,
                                 dist_fit=True, rad_prior=False, seed=4)
    assert len(out) == 24
    cs = np.loadtxt(tmp_path / 'optimize_cs.txt')
    pars = np.loadtxt(tmp_path / 'optimize_res.txt')
    assert cs.shape == (24,) and pars.shape == (24, 6)
    for line, best, ch in out:
        assert best <= ch.savechi[0] and np.all(np.diff(ch.savechi) <= 0)   # running best never increases
    assert (tmp_path / 'params0.txt').exists() and (tmp_path / 'chisq23.txt').exists()


def test_spectra_longer_than_lds_use_the_global_model_vector():
    """21,951 pixels (the size of the reference's Data/synth_spec_3850_3600.txt) do not fit the 160 KiB LDS:
    the kernel variant that keeps the model vector in global memory must give the same numbers."""
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd import bands
    from oracle import mft6_oracle as orc
    c = golden_case('B')
    npix = 21951
    rng = np.random.default_rng(8)
    wl_um = np.sort(rng.uniform(0.5499, 2.3991, npix))
    data = [wl_um, 1.0 + 0.1 * rng.normal(size=npix)]
    err = np.full(npix, 0.1)
    r = [wl_um.min(), wl_um.max()]
    eng = Engine(0)
    eng.stage_specs(c.specs)
    eng.stage_problem(data, err, c.fr, r, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=2,
                      bands=bands.make_bands(c.tables, *c.vega))
    th = c.theta[:5]
    got = eng.loglikelihood(th)
    want = np.array([orc.loglikelihood(list(t), c.fr, 2, data, err, r, c.specs, c.ctm, c.ptm, c.tmi, c.tma, c.matrix,
                                       bandlib=c.bandlib) for t in th])
    assert rel_err(got, want).max() < TIGHT
    assert np.array_equal(eng.loglikelihood(th[::-1]), got[::-1])


def test_device_resident_sampler_walks_the_same_chain_as_the_host_loop():
    """f2 on the device: same seed -> the GPU-resident stretch-move loop (msx_sampler_run) and the host-driven
    loop over the same fused log-posterior give bit-identical chains, log-probs and acceptance counts."""
    import time
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler, EnsembleSampler
    c = golden_case('B')
    eng = make_engine(c, rad_prior=False)
    rng = np.random.default_rng(3)
    nw = 64
    p0 = c.theta[0] + rng.normal(size=(nw, 6)) * np.array([30, 30, 0.02, 0.02, 0.02, 2e-5])
    host = EnsembleSampler(nw, 6, eng.logposterior, vectorize=True, seed=11)
    t0 = time.time()
    hs = host.run_mcmc(p0, 70)
    t_host = time.time() - t0
    dev = DeviceEnsembleSampler(nw, 6, eng, seed=11, chunk=32)   # 70 = 32 + 32 + 6: exercises chunking
    t0 = time.time()
    ds = dev.run_mcmc(p0, 70)
    t_dev = time.time() - t0
    assert np.array_equal(dev.chain, host.chain)
    assert np.array_equal(dev.get_log_prob(), host.get_log_prob())
    assert np.array_equal(dev.acceptance_fraction, host.acceptance_fraction)
    assert np.array_equal(ds.coords, hs.coords) and dev.acceptance_fraction.mean() > 0.05
    print('70 steps x 64 walkers: host loop {:.1f} ms, device-resident {:.1f} ms'.format(t_host * 1e3, t_dev * 1e3))
    # proposals that leave the prior box are rejected on the device: a chain started inside stays inside
    ok = p0.copy()
    ok[:, 1] = np.clip(ok[:, 1], 3001.0, None)
    ok[:, 2] = np.clip(ok[:, 2], 1e-3, None)
    s2 = DeviceEnsembleSampler(nw, 6, eng, seed=5)
    st = s2.run_mcmc(ok, 25)
    flat = s2.get_chain(flat=True)
    assert np.all(np.isfinite(st.log_prob)) and flat[:, 1].min() >= 3000.0 and flat[:, 2].min() >= 0.0


def test_device_resident_sampler_against_the_oracle_stretch_move():
    """Independent pin of f2 on the device: the fused kernel's proposal + accept lines against the walker-by-walker
    restatement in oracle/stretch_move.py driving the ORACLE's logposterior, from the same random numbers.  The
    coordinates depend on the log-probabilities only through accept decisions, so the chains must agree exactly;
    the log-probabilities agree to the parity tolerance."""
    from oracle import stretch_move as osm
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler, EnsembleSampler
    c = golden_case('B')
    eng = make_engine(c, rad_prior=False)
    rng = np.random.default_rng(12)
    nw, nsteps = 16, 10
    p0 = c.theta[0] + rng.normal(size=(nw, 6)) * np.array([30, 30, 0.02, 0.02, 0.02, 2e-5])
    p0[:, 1] = np.clip(p0[:, 1], 3001.0, None)
    dev = DeviceEnsembleSampler(nw, 6, eng, seed=31, chunk=4)
    dev.run_mcmc(p0, nsteps)
    twin = EnsembleSampler(nw, 6, None, vectorize=True, seed=31)
    sidx, cidx, partner, zz, zfac, logu = twin._draw_steps(nsteps)
    f = lambda q: np.array([oracle_logpost(c, t) for t in q])  # noqa: E731
    chain, lpc, nacc = osm.run_chain(p0, f(p0), (sidx, cidx, partner, zz, logu), f)
    assert np.array_equal(dev.get_chain(), chain)
    assert rel_err(dev.get_log_prob(), lpc).max() < TIGHT
    assert np.array_equal(dev.acceptance_fraction, nacc / nsteps) and 0 < nacc.sum() < nw * nsteps


def test_device_resident_sampler_statistics():
    """Moments / acceptance of DeviceEnsembleSampler itself: two device-resident runs from different seeds and a
    host-driven run sample the same posterior, so their pooled means must agree within a few standard errors and
    the acceptance fraction must sit where the stretch move's does for a 6-dimensional target."""
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler, EnsembleSampler
    c = golden_case('B')
    eng = make_engine(c, rad_prior=False)
    rng = np.random.default_rng(2)
    nw = 64
    p0 = c.theta[0] + rng.normal(size=(nw, 6)) * np.array([5, 5, 0.005, 0.005, 0.005, 5e-6])
    p0[:, 1] = np.clip(p0[:, 1], 3001.0, None)
    runs = []
    for seed, cls in ((1, DeviceEnsembleSampler), (2, DeviceEnsembleSampler), (3, None)):
        s = cls(nw, 6, eng, seed=seed, chunk=64) if cls else EnsembleSampler(nw, 6, eng.logposterior, vectorize=True, seed=seed)
        st = s.run_mcmc(p0, 400)
        s.reset()
        s.run_mcmc(st, 600)
        flat = s.get_chain(flat=True)
        runs.append((flat.mean(0), flat.std(0), s.acceptance_fraction.mean(), s.get_autocorr_time(quiet=True)))
    for m, sd, acc, tau in runs:
        assert 0.1 < acc < 0.8, acc
    m0, sd0, _, tau0 = runs[0]
    neff = nw * 600 / max(np.nanmax(tau0), 1.0)
    for m, sd, _, _ in runs[1:]:
        z = np.abs(m - m0) / (np.maximum(sd0, sd) / np.sqrt(neff / 2.0))
        assert z.max() < 6.0, z
        assert np.all(sd / sd0 < 2.0) and np.all(sd0 / sd < 2.0)


def test_sharded_device_sampler_on_one_rank_walks_the_fused_chain():
    """The sharded form's three device steps per half-step (block evaluation with the accept deferred, the
    all-gather -- a no-op at world size 1 --, the apply kernel) against the fully fused single-launch form: same
    chain, log-probabilities and acceptance counts, bit for bit, including rejected proposals; and a walker error
    surfaces through the NaN payload."""
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    c = golden_case('B')
    eng = make_engine(c, rad_prior=False)
    rng = np.random.default_rng(6)
    nw = 48
    p0 = c.theta[0] + rng.normal(size=(nw, 6)) * np.array([30, 30, 0.02, 0.02, 0.02, 2e-5])
    fused = DeviceEnsembleSampler(nw, 6, eng, seed=13, chunk=16)
    fs = fused.run_mcmc(p0, 40)
    shard = DeviceEnsembleSampler(nw, 6, eng, seed=13, chunk=16, shard=(0, 1))
    ss = shard.run_mcmc(p0, 40)
    assert np.array_equal(shard.chain, fused.chain)
    assert np.array_equal(shard.get_log_prob(), fused.get_log_prob())
    assert np.array_equal(shard.acceptance_fraction, fused.acceptance_fraction)
    assert np.array_equal(ss.coords, fs.coords) and 0.05 < shard.acceptance_fraction.mean() < 0.95
    # the same with the library's RCCL communicator in place (one rank): the all-gather is really enqueued, from C,
    # on the compute stream between the block evaluation and the apply kernel
    eng.ctx.comm_init(eng.ctx.comm_unique_id(), 0, 1)
    coll = DeviceEnsembleSampler(nw, 6, eng, seed=13, chunk=16, shard=(0, 1))
    coll.run_mcmc(p0, 40)
    assert np.array_equal(coll.chain, fused.chain) and np.array_equal(coll.get_log_prob(), fused.get_log_prob())
    # likelihood mode has no prior box: a proposal outside the isochrone table is an error status, not a value
    like = DeviceEnsembleSampler(nw, 6, eng, mode='loglikelihood', seed=2, chunk=8, shard=(0, 1))
    wide = p0.copy()
    wide[:, 1] = 2905.0 + np.abs(rng.normal(size=nw)) * 3      # stretch moves will step below the table's 2900 K
    with pytest.raises(ValueError):
        like.run_mcmc(wide, 60)


def test_pipelined_sampler_entry_points_guard_their_arguments():
    """msx_sampler_begin/_enqueue/_collect/_end: indices that would be dereferenced on the device are range-checked
    on the host, slots cannot be overwritten or collected twice, and a run continued from a State is the same
    chain as an uninterrupted one."""
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    c = golden_case('B')
    eng = make_engine(c, rad_prior=False)
    rng = np.random.default_rng(4)
    nw = 32
    p0 = c.theta[0] + rng.normal(size=(nw, 6)) * np.array([30, 30, 0.02, 0.02, 0.02, 2e-5])
    a = DeviceEnsembleSampler(nw, 6, eng, seed=2, chunk=16)
    a.run_mcmc(p0, 30)
    b = DeviceEnsembleSampler(nw, 6, eng, seed=2, chunk=16)
    st = b.run_mcmc(p0, 12)
    b.run_mcmc(st, 18)
    assert np.array_equal(a.chain, b.chain) and np.array_equal(a.acceptance_fraction, b.acceptance_fraction)

    ctx = eng.ctx
    lp = eng.logposterior(p0)
    draws = list(a._draw_steps(3))
    with pytest.raises(RuntimeError, match='msx_sampler_begin first'):
        ctx._smp_shape = (nw, 6)
        ctx.sampler_enqueue(0, *draws)
    ctx.sampler_begin(_lib.MODE_LOGPOST, p0, lp, 4)
    try:
        bad = [x.copy() for x in draws]
        bad[2][1, 0, 3] = nw // 2          # partner index one past the half
        with pytest.raises(RuntimeError, match='out of range'):
            ctx.sampler_enqueue(0, *bad)
        bad = [x.copy() for x in draws]
        bad[0][0, 1, 0] = -1               # active walker index
        with pytest.raises(RuntimeError, match='out of range'):
            ctx.sampler_enqueue(0, *bad)
        with pytest.raises(RuntimeError, match='bad arguments'):
            ctx.sampler_enqueue(0, *a._draw_steps(5))   # more steps than the slots were sized for
        with pytest.raises(RuntimeError, match='nothing enqueued'):
            ctx.sampler_collect(0, 3)
        ctx.sampler_enqueue(0, *draws)
        with pytest.raises(RuntimeError, match='not collected'):
            ctx.sampler_enqueue(0, *draws)
        chain, lpc, nacc, worst = ctx.sampler_collect(0, 3)
        assert worst == 0 and chain.shape == (3, nw, 6) and np.all(nacc <= 3) and nacc.sum() > 0
        coords, logp = ctx.sampler_end(want_state=True)
        assert np.array_equal(coords, chain[-1]) and np.array_equal(logp, lpc[-1])
        assert np.array_equal(eng.logposterior(coords), logp)   # the resident log-probs are those of the coords
    finally:
        ctx.sampler_end()                   # idempotent


def test_end_to_end_fit_recovers_the_truth(tmp_path, monkeypatch):
    """examples/fit_synthetic.py: loader -> optimiser -> device-resident sampler -> samples.txt, like the
    reference's main() minus plotting.  The posterior median must land on the injected parameters."""
    import importlib.util
    import sys as _sys
    spec = importlib.util.spec_from_file_location('fit_synthetic', common.ROOT + '/examples/fit_synthetic.py')
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    monkeypatch.setattr(_sys, 'argv', ['fit_synthetic.py', '--out', str(tmp_path / 'fit'), '--nwalk', '96', '--nstep', '40',
                                       '--nburn', '300', '--nsteps', '1500'])
    truth, med, samples = mod.main()
    assert samples.shape[1] == 6 and (tmp_path / 'fit' / 'samples.txt').exists()
    assert (tmp_path / 'fit' / 'optimize_res.txt').exists() and (tmp_path / 'fit' / 'grid_cache.npz').exists()
    # the primary dominates the spectrum: its Teff is recovered to well within a node spacing; the secondary
    # is only constrained through one contrast and the blend, the parallax by its Gaussian prior; the absolute
    # radius is degenerate here (median-normalised spectrum, no photometry) and is not checked
    assert abs(med[0] - truth[0]) < 60 and abs(med[1] - truth[1]) < 350
    assert abs(med[5] - truth[5]) < 1e-4


@pytest.mark.parametrize('rad_prior', [False, True])
def test_dist_fit_false_branch_matches_reference_golden(rad_prior):
    """logprior / logposterior with dist_fit=False (mft6.py:1275-1327): no parallax or R1 <= 1.5 bounds, a
    shorter Gaussian-prior list (here with Teff_1, A_V and R1 priors switched on)."""
    c = golden_case('A')
    g = c.g
    m = _dropin(c)
    th = g['theta_nodist']
    prior = list(g['prior_nodist'])
    args = [c.fr, 2, 0, c.data, c.err, 1700, c.r, c.specs, c.ctm, c.ptm, c.tmi, c.tma, None, c.tmin, c.tmax, c.matrix, 10.0,
            20.0]
    tag = 'radprior' if rad_prior else 'noradprior'
    got = m.logposterior(th, *args, prior=prior, a=True, dist_fit=False, rad_prior=rad_prior)
    want = g['A_nodist_logpost_' + tag]
    assert np.array_equal(np.isinf(got), np.isinf(want)) and rel_err(got, want).max() < TIGHT
    lp = m.logprior(th, 2, 0, c.tmin, c.tmax, c.matrix, 10.0, 20.0, prior=prior, ext=True, dist_fit=False,
                    rad_prior=rad_prior)
    wantp = g['A_nodist_logprior_' + tag]
    assert np.array_equal(np.isinf(lp), np.isinf(wantp)) and rel_err(lp, wantp).max() < 1e-12
    assert np.isfinite(want[10]) and np.isfinite(want[11])   # R1 = 1.7 and plx = 0.3 pass without dist_fit


@pytest.mark.parametrize('rad_prior', [False, True])
def test_triple_dist_fit_false_branch_matches_reference_golden(rad_prior):
    """The last prior branch: ndim 8 with dist_fit=False (mft6.py:1397-1455).  Gates (:1411): Teff box, the two RATIOS
    >= 0.05 -- R1 is not tested --, plx >= 0, A_V >= 0; Gaussian terms for Teff x 3, A_V, R1 and ratio 2 only
    (:1425-1442).  Through the drop-in signatures, against the reference's own logprior / logposterior."""
    c = golden_case('C')
    g = c.g
    m = _dropin(c)
    th = g['theta3_nodist']
    prior = list(g['prior3_nodist'])
    args = [c.fr, 3, 0, c.data, c.err, 1700, c.r, c.specs, c.ctm, c.ptm, c.tmi, c.tma, None, c.tmin, c.tmax, c.matrix, 10.0,
            20.0]
    tag = 'radprior' if rad_prior else 'noradprior'
    got = m.logposterior(th, *args, prior=prior, a=True, dist_fit=False, rad_prior=rad_prior)
    want = g['C_nodist_logpost_' + tag]
    assert np.array_equal(np.isinf(got), np.isinf(want)) and rel_err(got, want).max() < TIGHT
    lp = m.logprior(th, 3, 0, c.tmin, c.tmax, c.matrix, 10.0, 20.0, prior=prior, ext=True, dist_fit=False,
                    rad_prior=rad_prior)
    wantp = g['C_nodist_logprior_' + tag]
    assert np.array_equal(np.isinf(lp), np.isinf(wantp)) and rel_err(lp, wantp).max() < 1e-12
    assert np.isfinite(want[10]) and np.isfinite(want[11])   # R1 = 0.03 and plx = 0.3 pass without dist_fit
    assert np.all(np.isinf(want[12:]))                       # ratio 2, ratio 3, plx < 0, A_V < 0, Teff outside


def test_nospec_variant_matches_mft6_nospec_golden():
    """The mft6_nospec.py likelihood (spectrum term commented out, mft6_nospec.py:1163-1196) is a flag on the
    same kernel; golden values come from the reference's mft6_nospec.py itself."""
    c = golden_case('B')
    m = _dropin(c)
    m.set_spectrum_term(False)
    try:
        args = [c.fr, 2, 0, c.data, c.err, 1700, c.r, c.specs, c.ctm, c.ptm, c.tmi, c.tma, None, c.matrix]
        got = m.loglikelihood(c.theta[:12], *args)
        assert rel_err(got, c.g['B_nospec_loglike']).max() < 1e-12
    finally:
        m.set_spectrum_term(True)
    again = m.loglikelihood(c.theta[:12], *args)
    assert rel_err(again, c.g['B_loglike'][:12]).max() < TIGHT


def test_randomised_edge_walkers_against_oracle(engB):
    """Seeded fuzz over the whole prior box plus deliberately awkward values: Teff exactly on nodes, exactly
    half-way between nodes (find_nearest ties), logg landing near nodes, A_V = 0 and tiny, box edges."""
    c = golden_case('B')
    rng = np.random.default_rng(2024)
    n = 160
    th = np.column_stack([rng.uniform(3000, 4200, n), rng.uniform(3000, 4200, n), rng.uniform(0, 1.0, n),
                          rng.uniform(0.05, 1.5, n), rng.uniform(0.05, 1.2, n), rng.uniform(1 / 3000, 1 / 4, n)])
    nodes = np.arange(3000.0, 4300.0, 100.0)
    th[:20, 0] = rng.choice(nodes, 20)                       # on-node primaries
    th[20:40, 1] = rng.choice(nodes[:-1], 20) + 50.0         # exact ties between two nodes
    th[40:50, 2] = 0.0                                       # no reddening branch
    th[50:60, 2] = 1e-12
    th[60:64, 0] = [3000.0, 4200.0, 3000.0, 4200.0]          # box edges are inside (strict comparisons)
    th[64:68, 3] = [0.05, 1.5, 0.05, 1.5]
    th[68:70, 5] = [1 / 3000, 1 / 4]
    got = engB.logposterior(th)
    want = np.array([oracle_logpost(c, t) for t in th])
    assert np.array_equal(np.isinf(got), np.isinf(want))
    assert rel_err(got, want).max() < TIGHT
    ll = engB.loglikelihood(th)
    wl = np.array([oracle_loglike(c, t) for t in th])
    assert rel_err(ll, wl).max() < TIGHT


def test_resampled_tables_stay_at_rounding_level_under_heavy_extinction():
    """The blend reads, per grid node and pixel, R = lo + (hi - lo) t (float64) and H = hi t (float32) instead of
    the two model samples (blend.h): H only ever enters multiplied by e_hi / e_lo - 1 ~ 4e-5 A_V.  Its float32
    rounding must stay at float64 rounding level in the log-likelihood even at A_V = 3, thirty times the example
    run's extinction -- against the oracle, which blends, reddens and resamples like the reference."""
    c = golden_case('B')
    eng = make_engine(c, with_prior=False)
    th = np.repeat(c.theta[:6], 4, axis=0)
    th[:, 2] = np.tile([0.0, 0.3, 1.0, 3.0], 6)
    got = eng.loglikelihood(th)
    want = np.array([oracle_loglike(c, t) for t in th])
    e = rel_err(got, want)
    print('resampled tables, A_V in {0, 0.3, 1, 3}: max relative deviation from the oracle', e.max())
    assert e.max() < 1e-11
    # 12 bytes per node-pixel are in use; a workgroup with a CU to itself keeps u and the data flux in LDS for the chi^2 pass
    if not any(k in os.environ for k in ('MSX_PAIR_MIN', 'MSX_LINKED')):   # (the variants AUTO takes by default)
        assert eng.ctx.bytes_per_eval(1000) == 700 * (12 * 8 + 12 + 16 + 24) + 8 * 6 + 12
        assert eng.ctx.bytes_per_eval(64) == 700 * (12 * 8 + 12 + 16 + 8) + 8 * 6 + 12
        # ... and from 3,072 walkers on (12 per CU) two walkers of one grid cell share every load (+ the planner's 128-byte record)
        assert eng.ctx.bytes_per_eval(100000) == 700 * (12 * 8 + 12 + 16 + 24) // 2 + 128 + 8 * 6 + 12


def test_fuzzed_problems_against_the_oracle():
    """Randomised problems on the golden grid: pixel counts from 3 to 1500 (unsorted wavelengths, ragged against
    every workgroup size), random errors, with / without photometry, prior list, radius prior -- log-posterior of
    ten walkers each against the oracle."""
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd import bands
    from oracle import mft6_oracle as orc
    c = golden_case('B')
    bl = bands.make_bands(c.tables, *c.vega)
    eng = Engine(0)
    eng.stage_specs(c.specs)
    rng = np.random.default_rng(2024)
    lo, hi = float(np.min(c.data[0])), float(np.max(c.data[0]))
    worst = 0.0
    for case in range(40):
        npix = int(rng.choice([3, 5, 63, 64, 65, 255, 257, 511, 700, 1023, 1500])) if case < 11 else int(rng.integers(3, 1500))
        wl = rng.uniform(lo, hi, size=npix)
        data = [wl, 1.0 + 0.1 * rng.normal(size=npix)]
        err = rng.uniform(0.01, 0.2, size=npix)
        r = [wl.min(), wl.max()]
        phot = bool(rng.integers(0, 2))
        rad_prior = bool(rng.integers(0, 2))
        with_prior = bool(rng.integers(0, 2))
        ptm = c.ptm if phot else [[], [], [], []]
        fr = list(c.fr) if phot else [c.fr[0], c.fr[1], c.fr[2], np.zeros(0), [], np.array([])]
        tmi, tma = common.tm_extrema(c.ctm, ptm)
        prior = c.prior if with_prior else 0
        eng.stage_problem(data, err, fr, r, c.ctm, ptm, tmi, tma, c.matrix, nspec=2, bands=bl,
                          av_table=common.av_table_exact(), tmin=c.tmin, tmax=c.tmax, prior=prior, rad_prior=rad_prior)
        th = c.theta[rng.choice(len(c.theta), size=10, replace=False)]
        got = eng.logposterior(th)
        want = np.array([orc.logposterior(list(t), fr, 2, data, err, r, c.specs, c.ctm, ptm, tmi, tma, c.tmin, c.tmax,
                                          c.matrix, common.av_prior, prior=prior, rad_prior=rad_prior,
                                          bandlib=c.bandlib) for t in th])
        assert np.array_equal(np.isinf(got), np.isinf(want)), (case, npix)
        e = rel_err(got, want).max()
        worst = max(worst, float(e))
        assert e < TIGHT, (case, npix, phot, rad_prior, with_prior, e)
    print('fuzz: worst relative deviation from the oracle', worst)


def test_brackets_at_and_beyond_the_edges_of_the_node_lists():
    """The lane-parallel brackets of the recipe (csrc/recipe.h) in the corners no interval owns: a value below the
    first node (the reference's unchecked index -1 wraps to the LAST node, mft6.py:467-477), exactly on the first /
    last node, beyond the last node (IndexError) -- for Teff and for logg, against the oracle."""
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd import bands
    from oracle import mft6_oracle as orc
    c = golden_case('B')
    bl = bands.make_bands(c.tables, *c.vega)

    def engine_for(keep):
        specs = {k: v for k, v in c.specs.items() if k == 'wl' or keep(*[float(x) for x in k.split(',')])}
        eng = Engine(0)
        eng.stage_specs(specs)
        eng.stage_problem(c.data, c.err, c.fr, c.r, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=2, bands=bl,
                          av_table=common.av_table_exact(), tmin=c.tmin, tmax=c.tmax, prior=c.prior)
        return eng, specs

    def want(specs, t):
        return orc.loglikelihood(list(t), c.fr, 2, c.data, c.err, c.r, specs, c.ctm, c.ptm, c.tmi, c.tma, c.matrix,
                                 bandlib=c.bandlib)

    base = c.theta[0].copy()
    # ---- Teff nodes 3200 .. 4000 only (the isochrone and the prior box still span 3000 .. 4200)
    eng, specs = engine_for(lambda t, g: 3200.0 <= t <= 4000.0)
    cases = []
    for t1, t2 in [(3150.0, 3650.0), (3650.0, 3150.0), (3199.999, 3200.0), (3200.0, 4000.0), (4000.0, 3999.5), (3100.0, 3120.0)]:
        th = base.copy()
        th[0], th[1] = t1, t2
        cases.append(th)
    th = np.array(cases)
    got = eng.loglikelihood(th)
    exp = np.array([want(specs, t) for t in th])
    assert np.all(np.isfinite(exp)) and rel_err(got, exp).max() < TIGHT, (got, exp)
    for t1, t2 in [(4000.5, 3650.0), (3650.0, 4199.0)]:
        bad = base.copy()
        bad[0], bad[1] = t1, t2
        with pytest.raises(IndexError):
            want(specs, bad)
        with pytest.raises(IndexError):
            eng.loglikelihood(bad)
    # ---- logg nodes 5.0, 5.5 only: the isochrone's logg drops below 5.0 above ~4030 K (wrap), lies inside below
    eng, specs = engine_for(lambda t, g: g >= 5.0)
    cases = []
    for t1, t2 in [(4100.0, 3500.0), (3500.0, 4150.0), (4180.0, 4060.0), (3850.0, 3325.0)]:
        th = base.copy()
        th[0], th[1] = t1, t2
        cases.append(th)
    th = np.array(cases)
    got = eng.loglikelihood(th)
    exp = np.array([want(specs, t) for t in th])
    assert np.all(np.isfinite(exp)) and rel_err(got, exp).max() < TIGHT, (got, exp)
    # ---- one logg node: every bracket degenerates to it
    eng, specs = engine_for(lambda t, g: g == 5.5)
    got = eng.loglikelihood(c.theta[:6])
    exp = np.array([want(specs, t) for t in c.theta[:6]])
    assert rel_err(got, exp).max() < TIGHT
    # ---- logg nodes 4.0, 4.5 only: logg ~ 5.1 lies beyond the last node -> IndexError
    eng, specs = engine_for(lambda t, g: g <= 4.5)
    with pytest.raises(IndexError):
        want(specs, base)
    with pytest.raises(IndexError):
        eng.loglikelihood(base)


def test_register_recipe_on_a_dense_grid_with_holes():
    """40 Teff x 20 logg nodes (the register-resident recipe's presence BITS beyond the first few, Teff lanes up to
    39; round 1's byte table stopped at 128 nodes) with a few nodes missing: log-posterior against the oracle, and
    KeyError exactly where the oracle raises it."""
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd import bands, synth
    from oracle import mft6_oracle as orc
    c = golden_case('B')
    teffs = np.arange(3000, 4200, 30)
    loggs = 4.0 + 0.075 * np.arange(20)
    wl = np.arange(5300.0, 9700.0, 0.5)
    flux = synth.make_grid(teffs, loggs, wl, nlines=150, seed=5)
    specs = synth.grid_to_specs(teffs, loggs, wl, flux)
    holes = [(3630, loggs[14]), (3660, loggs[15]), (3300, loggs[13])]
    for t, g in holes:
        del specs['{}, {}'.format(int(t), float(g))]
    rng = np.random.default_rng(12)
    npix = 900
    dwl = np.sort(rng.uniform(0.58, 0.88, npix))
    data = [dwl, 1.0 + 0.05 * rng.normal(size=npix)]
    err = rng.uniform(0.01, 0.05, size=npix)
    r = [dwl.min(), dwl.max()]
    ctm = [[list(np.linspace(6000.0, 9500.0, 60))], [list(0.9 * np.ones(60))], [0], [7750.0]]
    ptm = [[], [], [], []]
    fr = [[2.4], [0.05], np.array(['x']), np.zeros(0), [], np.array([])]
    tmi, tma = 6000.0, 9500.0
    eng = Engine(0)
    eng.stage_specs(specs)
    eng.stage_problem(data, err, fr, r, ctm, ptm, tmi, tma, c.matrix, nspec=2, bands=bands.make_bands(c.tables, *c.vega),
                      av_table=common.av_table_exact(), tmin=3000.0, tmax=4170.0, prior=c.prior)
    n = 48
    th = np.column_stack([rng.uniform(3005, 4165, n), rng.uniform(3005, 4165, n), rng.uniform(0, 0.6, n),
                          rng.uniform(0.1, 1.2, n), rng.uniform(0.1, 1.0, n), rng.uniform(1 / 2000, 1 / 50, n)])
    th[:6, 0] = teffs[[0, 5, 17, 30, 38, 39]]           # on nodes, including the first and the last
    th[6:10, 1] = teffs[[3, 11, 21, 35]] + 15.0          # ties
    th[10, 0], th[11, 1], th[12, 0] = 3640.0, 3650.0, 3310.0   # cells that touch the holes
    got_vals, want_vals, bad = [], [], 0
    for t in th:
        try:
            w = orc.logposterior(list(t), fr, 2, data, err, r, specs, ctm, ptm, tmi, tma, 3000.0, 4170.0, c.matrix,
                                 common.av_prior, prior=c.prior, bandlib=c.bandlib)
        except KeyError:
            bad += 1
            with pytest.raises(KeyError):
                eng.logposterior(t)
            continue
        got_vals.append(eng.logposterior(t))
        want_vals.append(w)
    got_vals, want_vals = np.array(got_vals), np.array(want_vals)
    assert bad >= 2 and len(got_vals) >= 30
    assert np.array_equal(np.isinf(got_vals), np.isinf(want_vals))
    assert rel_err(got_vals, want_vals).max() < TIGHT
    # the same walkers in one launch: the good ones keep their values whatever their neighbours raise
    good = np.array([t for t in th if True])
    st = eng.ctx.logprob_batch(good, __import__('mcmc_spec_amd._lib', fromlist=['x']).MODE_LOGPOST)[1]
    assert int((st == 0).sum() + (st == 1).sum()) == len(got_vals)


@pytest.mark.parametrize('which', ['B', 'C'])
def test_statuses_and_values_beyond_the_box(which):
    """loglikelihood over a box LARGER than the grid and the isochrone (binaries and triples): the exception class of
    every walker (Teff outside the isochrone -> ValueError on any star first, beyond the last node -> IndexError,
    missing node -> KeyError) and the values of the rest against the oracle.  Walkers below the grid's first node are
    compared loosely: the reference's wrapped bracket (index -1) extrapolates between the first and the last node, the
    model crosses zero near 2907 K and the likelihood is singular there (observed: <= 6e-6 relative on values of 1e10)."""
    from oracle import mft6_oracle as orc
    from mcmc_spec_amd import _lib
    c = golden_case(which)
    ns = c.nspec
    eng = make_engine(c, rad_prior=(which == 'C'))
    rng = np.random.default_rng(31 + ns)
    n = 500
    cols = [rng.uniform(2850, 4350, n) for _ in range(ns)] + [rng.uniform(0.0, 1.2, n)] + \
           [rng.uniform(0.03, 1.6, n) for _ in range(ns)] + [rng.uniform(1 / 3200, 1 / 3.5, n)]
    th = np.column_stack(cols)
    th[:8, 0], th[:8, 1] = 4325.0, 2874.0            # IndexError on the primary, ValueError on the secondary: ValueError
    exp_st = np.zeros(n, dtype=np.int32)
    want = np.full(n, np.nan)
    for i, t in enumerate(th):
        try:
            want[i] = orc.loglikelihood(list(t), c.fr, ns, c.data, c.err, c.r, c.specs, c.ctm, c.ptm, c.tmi, c.tma, c.matrix,
                                        bandlib=c.bandlib)
        except KeyError:
            exp_st[i] = _lib.W_KEYERROR
        except IndexError:
            exp_st[i] = _lib.W_INDEXERROR
        except ValueError:
            exp_st[i] = _lib.W_VALUEERROR
    got, st = eng.ctx.logprob_batch(th, _lib.MODE_LOGLIKE)
    assert np.array_equal(st, exp_st), {int(k): int((st == k).sum()) for k in np.unique(st)}
    assert (exp_st == _lib.W_VALUEERROR).sum() >= 8 and (exp_st == _lib.W_INDEXERROR).sum() >= 20
    ok = exp_st == 0
    inside = ok & np.all(th[:, :ns] >= 3000.0, axis=1)
    assert inside.sum() >= 100 and rel_err(got[inside], want[inside]).max() < TIGHT
    wrapped = ok & ~inside
    if wrapped.any():
        assert rel_err(got[wrapped], want[wrapped]).max() < 1e-4


@pytest.mark.parametrize('npix', [5700, 5800, 6000, 6271, 6400])
def test_lds_staged_variant_is_only_taken_where_it_fits(npix):
    """Around the spectrum length where model vector + u + data flux stop fitting the LDS beside the kernel's static
    part (the PF variants; the bound is asked of the compiled functions at msx_stage_problem): a launch of few walkers
    -- one workgroup per CU, the variant in question -- must work on either side of it and give the bits of a large
    launch (256-thread variant, nothing staged)."""
    from mcmc_spec_amd import bands
    from mcmc_spec_amd.engine import Engine
    c = golden_case('B')
    rng = np.random.default_rng(npix)
    wl = np.sort(rng.uniform(0.56, 0.89, npix))
    data = [wl, 1.0 + 0.05 * rng.normal(size=wl.size)]
    err = np.full(wl.size, 0.05)
    eng = Engine(0)
    eng.stage_specs(c.specs)
    eng.stage_problem(data, err, c.fr, [wl.min(), wl.max()], c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=2,
                      bands=bands.make_bands(c.tables, *c.vega))
    few = eng.loglikelihood(c.theta[:9])
    many = eng.loglikelihood(np.tile(c.theta[:9], (80, 1)))
    assert np.all(np.isfinite(few)) and np.array_equal(np.tile(few, 80), many)
    one = common.orc.loglikelihood(list(c.theta[0]), c.fr, 2, data, err, [wl.min(), wl.max()], c.specs, c.ctm, c.ptm,
                                   c.tmi, c.tma, c.matrix, bandlib=c.bandlib)
    assert rel_err(few[0], one) < TIGHT
