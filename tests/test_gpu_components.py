"""GPU: component grids -- one v sin i and limb darkening per star (DESIGN.md "Component grids"; include/msx.h,
msx_split_components).

A component grid holds one copy of every node row per star; star s of every walker reads copy s through the node
stride of the recipe.  Pinned here:
  * plumbing: split without rotation, every form gives the bits of the unsplit grid (the stride at every site);
  * equal rotation: the bits of today's single rotated grid;
  * unequal rotation: each copy is the NumPy restatement of pyasl.rotBroad (tests/rotbroad_numpy.py), the forms agree,
    and the likelihood is the oracle's with star s read from its own specs (tests/component_restatement.py);
  * the drop-ins, the loader and the refusals.
"""
import numpy as np
import pytest

import common
from common import golden_case, rel_err
import component_restatement as cr
import rotbroad_numpy as rb

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
MODES = ('LOGPOST', 'LOGLIKE', 'CHISQ', 'LOGPRIOR')


def _stage(eng, c, **kw):
    from mcmc_spec_amd import bands
    kw.setdefault('rad_prior', c.nspec == 3)
    eng.stage_problem(c.data, c.err, c.fr, c.r, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=c.nspec,
                      bands=bands.make_bands(c.tables, *c.vega), av_table=common.av_table_exact(), tmin=c.tmin,
                      tmax=c.tmax, prior=c.prior, **kw)


def golden_engines(which, **kw):
    """(plain, split): golden case `which` staged as it is and as a component grid of nspec unrotated copies."""
    from mcmc_spec_amd.engine import Engine
    key = ('comp_golden', which, tuple(sorted(kw.items())))
    if key not in common._cache:
        c = golden_case(which)
        a, b = Engine(0), Engine(0)
        a.stage_specs(c.specs)
        b.stage_specs(c.specs)
        b.ctx.split_components(c.nspec)
        _stage(a, c, **kw)
        _stage(b, c, **kw)
        common._cache[key] = (a, b)
    return common._cache[key]


def walkers(c, n, seed):
    """n walkers around the golden thetas (some outside the grid or the prior box: their status bits count too)."""
    rng = np.random.default_rng(seed)
    base = np.tile(c.theta, (n // len(c.theta) + 1, 1))[:n]
    sc = np.array([15.0] * c.nspec + [0.01] + [0.01] * c.nspec + [1e-5])
    return base + rng.normal(size=base.shape) * sc * (rng.random((n, 1)) < 0.75)


def raw(eng, th, mode, path):
    from mcmc_spec_amd import _lib
    eng.ctx.set_path(getattr(_lib, 'PATH_' + path))
    try:
        return eng.ctx.logprob_batch(th, getattr(_lib, 'MODE_' + mode))
    finally:
        eng.ctx.set_path(_lib.PATH_AUTO)


def same(a, b, th, mode, path='AUTO'):
    la, sa = raw(a, th, mode, path)
    lb, sb = raw(b, th, mode, path)
    return np.array_equal(la, lb, equal_nan=True) and np.array_equal(sa, sb)


# ---- plumbing: no rotation ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize('which', ['B', 'C'])
def test_split_grid_without_rotation_is_the_plain_grid_fused(which):
    c = golden_case(which)
    a, b = golden_engines(which)
    for n in (7, 256, 1000):
        th = walkers(c, n, seed=n)
        for mode in MODES:
            for path in ('FUSED', 'AUTO'):
                assert same(a, b, th, mode, path), (n, mode, path)
    lp, st = raw(a, walkers(c, 256, seed=256), 'LOGPOST', 'FUSED')
    assert np.isfinite(lp).sum() > 64 and (st == 0).sum() > 64


def test_split_grid_without_rotation_pair_form():
    c = golden_case('B')
    a, b = golden_engines('B')
    th = walkers(c, 2305, seed=5)
    for mode in ('LOGPOST', 'CHISQ'):
        assert same(a, b, th, mode, 'PAIR'), mode
    fused, pair = raw(b, th, 'LOGPOST', 'FUSED')[0], raw(b, th, 'LOGPOST', 'PAIR')[0]
    assert np.array_equal(fused, pair, equal_nan=True)


@pytest.mark.parametrize('which', ['B', 'C'])
def test_split_grid_without_rotation_no_spectrum_and_composite(which):
    c = golden_case(which)
    a, b = golden_engines(which, spectrum=False)
    th = walkers(c, 256, seed=3)
    for mode in ('LOGPOST', 'LOGLIKE'):
        assert same(a, b, th, mode, 'FUSED')
    a, b = golden_engines(which)
    from mcmc_spec_amd import staging
    t = c.theta[0]
    lg = staging.isochrone_logg(t[:c.nspec], c.matrix)
    rad = t[c.nspec + 1:2 * c.nspec + 1]
    for dist in (t[-1], False):
        ea, eb = a.make_composite(t[:c.nspec], lg, rad, dist), b.make_composite(t[:c.nspec], lg, rad, dist)
        assert all(np.array_equal(np.asarray(x), np.asarray(y)) for x, y in zip(ea, eb))


def test_split_grid_without_rotation_f32_storage():
    c = golden_case('B')
    a, b = golden_engines('B', store='f32')
    th = walkers(c, 256, seed=9)
    for mode in ('LOGPOST', 'LOGLIKE'):
        assert same(a, b, th, mode, 'FUSED')


def test_split_grid_without_rotation_optimiser():
    from mcmc_spec_amd import bands
    from mcmc_spec_amd.engine import Engine
    c = golden_case('B')
    a, b = Engine(0), Engine(0)
    for eng in (a, b):       # staged like the optimiser's own test (test_gpu_parity.py)
        eng.stage_specs(c.specs)
        if eng is b:
            eng.ctx.split_components(2)
        eng.stage_problem(c.data, c.err, c.fr, c.r, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=2,
                          bands=bands.make_bands(c.tables, *c.vega))
    st = c.g['D_start']
    ia, ib = a.ctx.opt_init(st[None, :]), b.ctx.opt_init(st[None, :])
    assert np.array_equal(ia[0], ib[0]) and np.array_equal(ia[1], ib[1])
    th = walkers(c, 64, seed=2)
    ch = np.zeros(len(th), dtype=np.int32)
    sa, sb = a.ctx.opt_step(th, ch), b.ctx.opt_step(th, ch)
    assert np.array_equal(sa[0], sb[0], equal_nan=True) and np.array_equal(sa[1], sb[1])


@pytest.mark.parametrize('which', ['B', 'C'])
def test_split_grid_without_rotation_device_sampler(which):
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    c = golden_case(which)
    a, b = golden_engines(which)
    good = c.theta[np.isfinite(a.logposterior(c.theta))]
    rng = np.random.default_rng(12)
    ndim = 2 * c.nspec + 2
    p0 = good[0] + rng.normal(size=(32, ndim)) * np.array([10.0] * c.nspec + [0.01] * (c.nspec + 1) + [1e-5])
    runs = []
    for eng in (a, b):
        dev = DeviceEnsembleSampler(32, ndim, eng, mode='logposterior', seed=4, chunk=8)
        dev.run_mcmc(p0, 17)
        runs.append(dev)
    assert np.array_equal(runs[0].get_chain(), runs[1].get_chain())
    assert np.array_equal(runs[0].get_log_prob(), runs[1].get_log_prob(), equal_nan=True)


# ---- the bench's workloads: rotation ----------------------------------------------------------------------------------
def bench_engines(npix, phot):
    """The bench workload (config 2: 4096 px; config 4: 16,384 px + photometry) and, on the same grid and data:
    'plain' (Gaussian only), 'rot' (one rotated grid), 'split' (two unrotated copies), 'equal' (two copies rotated
    alike), 'unequal' (two copies, rotated differently)."""
    from bench import build_workload
    from mcmc_spec_amd.engine import Engine
    key = ('comp_bench', npix, phot)
    if key not in common._cache:
        plain = Engine(0)
        W = build_workload(plain, npix, phot, keep_host_grid=True)
        out = {'plain': plain}
        for name, vs, ls in (('rot', 60.0, 0.6), ('split', (0, 0), (0, 0)), ('equal', (60.0, 60.0), (0.6, 0.6)),
                             ('unequal', (60.0, 12.0), (0.6, 0.3))):
            eng = Engine(0)
            eng.stage_grid(W['wl'], W['teffs'], W['loggs'], W['flux'])
            eng.broaden_grid_window(W['win'], W['resolution'], vsini=vs, limb=ls)
            restage(eng, W)
            out[name] = eng
        common._cache[key] = (out, W)
    return common._cache[key]


def restage(eng, W):
    from mcmc_spec_amd import bands, synth
    bl = bands.make_bands(W['tabs'], *W['vega'])
    eng.stage_problem(W['data'], W['err'], W['fr'], W['r'], W['ctm'], W['ptm'], W['tmi'], W['tma'], W['matrix'], nspec=2,
                      bands=bl, av_table=synth.make_av_table(), tmin=W['tmin'], tmax=W['tmax'], prior=W['prior'])


def bench_walkers(W, n, seed):
    from mcmc_spec_amd import synth
    return synth.draw_walkers(n, seed=seed, tmin=W['tmin'], tmax=W['tmax'])


def test_config2_split_and_equal_rotation_keep_the_bits():
    E, W = bench_engines(4096, False)
    for n, paths in ((256, ('FUSED', 'AUTO')), (2305, ('PAIR', 'AUTO'))):
        th = bench_walkers(W, n, seed=n)
        for path in paths:
            assert same(E['plain'], E['split'], th, 'LOGPOST', path), (n, path)
            assert same(E['rot'], E['equal'], th, 'LOGPOST', path), (n, path)
    lp = raw(E['rot'], th, 'LOGPOST', 'AUTO')[0]
    assert np.isfinite(lp).sum() > 2000 and not np.array_equal(lp, raw(E['plain'], th, 'LOGPOST', 'AUTO')[0])


def test_config4_linked_form_on_component_grids():
    E, W = bench_engines(16384, True)
    for n in (5, 128):
        th = bench_walkers(W, n, seed=40 + n)
        for path in ('LINKED', 'FUSED'):
            assert same(E['plain'], E['split'], th, 'LOGPOST', path), (n, path)
            assert same(E['rot'], E['equal'], th, 'LOGPOST', path), (n, path)
        fused, linked = raw(E['unequal'], th, 'LOGPOST', 'FUSED')[0], raw(E['unequal'], th, 'LOGPOST', 'LINKED')[0]
        assert np.array_equal(fused, linked, equal_nan=True) and np.isfinite(fused).sum() > n // 2


def test_unequal_rotation_copies_match_the_restatement():
    E, W = bench_engines(4096, False)
    wl = W['wl']
    inside = (wl >= min(W['win'])) & (wl <= max(W['win']))
    plain, uneq = E['plain'].ctx, E['unequal'].ctx
    nt, ng = len(W['teffs']), len(W['loggs'])
    rng = np.random.default_rng(1)
    check = {(int(rng.integers(nt)), int(rng.integers(ng))) for _ in range(6)} | {(0, 0), (nt - 1, ng - 1)}
    for it in range(nt):
        for ig in range(ng):
            gauss = plain.read_node(it, ig)
            for s, (vs, ls) in enumerate(((60.0, 0.6), (12.0, 0.3))):
                got = uneq.read_node_component(s, it, ig)
                assert np.array_equal(got[~inside], gauss[~inside]), (s, it, ig)   # outside the window: untouched
                if (it, ig) in check:
                    assert rel_err(got[inside], rb.rot_broad(wl[inside], gauss[inside], ls, vs)).max() <= 1e-12
    # copy 0 is the scalar rotation with (60, 0.6) bit for bit
    rot = E['rot'].ctx
    assert all(np.array_equal(uneq.read_node_component(0, it, ig), rot.read_node(it, ig)) for it, ig in check)
    # and read_node is copy 0
    assert np.array_equal(uneq.read_node(1, 2), uneq.read_node_component(0, 1, 2))


def test_a_copy_whose_pair_fails_the_condition_stays_gaussian_only():
    from mcmc_spec_amd.engine import Engine
    E, W = bench_engines(4096, False)
    eng = Engine(0)
    eng.stage_grid(W['wl'], W['teffs'], W['loggs'], W['flux'])
    eng.broaden_grid_window(W['win'], W['resolution'], vsini=(12.0, 0, 60.0), limb=(0.3, 0.6, 0.6))
    for it, ig in ((0, 0), (5, 2), (25, 3)):
        assert np.array_equal(eng.ctx.read_node_component(0, it, ig), E['unequal'].ctx.read_node_component(1, it, ig))
        assert np.array_equal(eng.ctx.read_node_component(1, it, ig), E['plain'].ctx.read_node(it, ig))
        assert np.array_equal(eng.ctx.read_node_component(2, it, ig), E['rot'].ctx.read_node(it, ig))


def test_unequal_rotation_forms_agree():
    E, W = bench_engines(4096, False)
    th = bench_walkers(W, 2305, seed=9)
    outs = [raw(E['unequal'], th, 'LOGPOST', p) for p in ('FUSED', 'PAIR', 'AUTO')]
    assert all(np.array_equal(outs[0][0], o[0], equal_nan=True) and np.array_equal(outs[0][1], o[1]) for o in outs)
    assert np.isfinite(outs[0][0]).sum() > 2000
    # it is neither of the single-rotation grids
    assert not np.array_equal(outs[0][0], raw(E['rot'], th, 'LOGPOST', 'AUTO')[0])


# ---- parity with the oracle, star s read from its own specs -------------------------------------------------------------
ROTATIONS = {'B': ((40.0, 8.0), (0.6, 0.3)), 'C': ((80.0, 0.0, 15.0), (0.6, 0.6, 0.4))}


def rotated_golden(which):
    """Golden case `which`, its grid broadened over the data window and rotated per star; the per-star specs read back."""
    from mcmc_spec_amd.engine import Engine
    key = ('comp_rot_golden', which)
    if key not in common._cache:
        c = golden_case(which)
        eng = Engine(0)
        eng.stage_specs(c.specs)
        wl_um = np.asarray(c.data[0])
        win = [np.floor(wl_um.min() * 1e4) - 20.0, np.ceil(wl_um.max() * 1e4) + 20.0]
        vs, ls = ROTATIONS[which]
        eng.broaden_grid_window(win, 1700, vsini=vs, limb=ls)
        _stage(eng, c)
        seq = []
        for s in range(c.nspec):
            d = {'wl': np.array(c.specs['wl'])}
            for it, t in enumerate(eng.grid['teff']):
                for ig, g in enumerate(eng.grid['logg']):
                    k = '{}, {}'.format(int(t), float(g))
                    if k in c.specs:
                        d[k] = eng.ctx.read_node_component(s, it, ig)
            seq.append(d)
        common._cache[key] = (eng, tuple(seq))
    return common._cache[key]


@pytest.mark.parametrize('which', ['B', 'C'])
def test_unequal_rotation_matches_the_oracle_restatement(which):
    c = golden_case(which)
    eng, seq = rotated_golden(which)
    assert not np.array_equal(seq[0][next(k for k in seq[0] if k != 'wl')], seq[-1][next(k for k in seq[0] if k != 'wl')])
    th = c.theta[:12]
    rp = c.nspec == 3
    got = eng.logposterior(th)
    want = np.array([cr.logposterior(list(t), c.fr, c.nspec, c.data, c.err, c.r, seq, c.ctm, c.ptm, c.tmi, c.tma, c.tmin,
                                     c.tmax, c.matrix, common.av_prior, prior=c.prior, rad_prior=rp, bandlib=c.bandlib)
                     for t in th])
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and fin.sum() >= 4
    assert rel_err(got[fin], want[fin]).max() < TIGHT
    # the likelihood alone: spectrum, contrasts and 6-band photometry
    got = eng.loglikelihood(th)
    want = np.array([cr.loglikelihood(list(t), c.fr, c.nspec, c.data, c.err, c.r, seq, c.ctm, c.ptm, c.tmi, c.tma, c.matrix,
                                      bandlib=c.bandlib) for t in th])
    fin = np.isfinite(want)
    assert np.array_equal(np.isfinite(got), fin) and rel_err(got[fin], want[fin]).max() < TIGHT
    # ... which is not the likelihood of either single grid
    one = [cr.loglikelihood(list(th[0]), c.fr, c.nspec, c.data, c.err, c.r, (seq[s],) * c.nspec, c.ctm, c.ptm, c.tmi,
                            c.tma, c.matrix, bandlib=c.bandlib) for s in (0, c.nspec - 1)]
    assert all(rel_err(got[0], o) > 1e-6 for o in one)


# ---- drop-ins and loader -------------------------------------------------------------------------------------------------
def _dropin(c):
    import mcmc_spec_amd.mft6 as m
    from mcmc_spec_amd import bands
    m.clear_cache()
    m.set_band_library(bands.make_bands(c.tables, *c.vega))
    m.set_av_prior(*common.av_table_exact())
    return m


@pytest.mark.parametrize('which', ['B', 'C'])
def test_dropins_take_one_specs_dict_per_star(which):
    c = golden_case(which)
    eng, seq = rotated_golden(which)
    m = _dropin(c)
    rp = c.nspec == 3
    th = c.theta[:12]
    args = [c.fr, c.nspec, 0, c.data, c.err, 1700, c.r, seq, c.ctm, c.ptm, c.tmi, c.tma, None]
    post = m.logposterior(th, *args, c.tmin, c.tmax, c.matrix, 10.0, 20.0, prior=c.prior, rad_prior=rp)
    assert np.array_equal(post, eng.logposterior(th))
    assert np.array_equal(m.loglikelihood(th, *args, c.matrix), eng.loglikelihood(th))
    t = c.theta[0]
    from mcmc_spec_amd import staging
    lg = staging.isochrone_logg(t[:c.nspec], c.matrix)
    rad = t[c.nspec + 1:2 * c.nspec + 1]
    got = m.make_composite(t[:c.nspec], lg, rad, t[-1], c.fr[2], c.fr[5], c.r, seq, c.ctm, c.ptm, c.tmi, c.tma, None,
                           nspec=c.nspec)
    want = cr.make_composite_components(t[:c.nspec], lg, rad, t[-1], c.fr[2], c.fr[5], c.r, seq, c.ctm, c.ptm, c.tmi,
                                        c.tma, nspec=c.nspec, bandlib=c.bandlib)
    assert rel_err(got[1], want[1]).max() < TIGHT and rel_err(got[2], want[2]).max() < TIGHT
    if len(c.fr[5]):
        assert rel_err(got[4], want[4]).max() < TIGHT
    # the device-resident sampler through the drop-in's arguments
    p0 = th[np.isfinite(post)][:1] + np.random.default_rng(3).normal(size=(16, 2 * c.nspec + 2)) * 1e-6
    s = m.device_sampler(16, 2 * c.nspec + 2, args + [c.tmin, c.tmax, c.matrix, 10.0, 20.0],
                         dict(prior=c.prior, rad_prior=rp), seed=2, chunk=4)
    s.run_mcmc(p0, 4)
    assert np.isfinite(s.get_log_prob()).all()
    # one dict keeps today's behaviour; dicts that do not match each other are refused
    one = m.loglikelihood(th, *(args[:7] + [c.specs] + args[8:]), c.matrix)
    assert not np.array_equal(one, eng.loglikelihood(th))
    bad = dict(seq[-1])
    bad.pop(next(k for k in bad if k != 'wl'))
    with pytest.raises(ValueError, match='keys'):
        m.loglikelihood(th, *(args[:7] + [seq[:-1] + (bad,)] + args[8:]), c.matrix)
    with pytest.raises(ValueError, match='nspec'):
        m.loglikelihood(th, *(args[:7] + [seq + (seq[0],) if c.nspec == 2 else seq[:2]] + args[8:]), c.matrix)
    m.clear_cache()


def test_loader_per_star_rotation_equals_scalar_calls_and_keeps_its_cache_apart(tmp_path):
    from mcmc_spec_amd import loader, synth
    import mcmc_spec_amd.mft6 as m
    gdir = synth.write_btsettl_text_grid(str(tmp_path / 'BT-Settl_M-0.0a+0.0'), seed=21)
    args = ([6000.0, 8000.0], [3000, 3200], [4, 5.5], [5000, 9000])
    cache = str(tmp_path / 'grid_cache.npz')
    m.clear_cache()
    one = [loader.spec_interpolator(*args, resolution=1700, grid_dir=gdir, vsini=vs, limb=ls)
           for vs, ls in ((60, 0.6), (10, 0.3), (0, 0.5))]
    per = loader.spec_interpolator(*args, resolution=1700, grid_dir=gdir, cache=cache, vsini=(60, 10, 0),
                                   limb=(0.6, 0.3, 0.5))
    assert isinstance(per, tuple) and len(per) == 3 and per.engine is not None
    for s in range(3):
        assert set(per[s]) == set(one[s]) and all(np.array_equal(per[s][k], one[s][k]) for k in one[s])
    # the cache: a scalar request is not served the per-star file, nor the per-star request another rotation's
    plain = loader.spec_interpolator(*args, resolution=1700, grid_dir=gdir, cache=cache, vsini=60, limb=0.6)
    assert not isinstance(plain, tuple) and all(np.array_equal(plain[k], one[0][k]) for k in plain)
    per2 = loader.spec_interpolator(*args, resolution=1700, grid_dir=gdir, cache=cache, vsini=(10, 60, 0),
                                    limb=(0.3, 0.6, 0.5))
    assert all(np.array_equal(per2[0][k], one[1][k]) and np.array_equal(per2[1][k], one[0][k]) for k in one[0])
    # ... and a per-star request served from its own cache file is what was written
    per3 = loader.spec_interpolator(*args, resolution=1700, grid_dir=gdir, cache=cache, vsini=(10, 60, 0),
                                    limb=(0.3, 0.6, 0.5))
    assert all(np.array_equal(per3[s][k], per2[s][k]) for s in range(3) for k in per2[s])
    assert per3.engine.ctx.ncomp == 3
    m.clear_cache()


# ---- refusals ------------------------------------------------------------------------------------------------------------
def test_refusals():
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.engine import Engine
    c = golden_case('B')
    eng = Engine(0)
    eng.stage_specs(c.specs)
    for bad in (0, 4, -1):
        with pytest.raises(ValueError, match='ncomp'):
            eng.ctx.split_components(bad)
    flux = np.zeros((4, len(eng.grid['teff']), len(eng.grid['logg']), 8))
    e2 = Engine(0)
    with pytest.raises(ValueError, match='ncomp'):
        e2.ctx.stage_grid_components(np.arange(8) * 0.2 + 5000, eng.grid['teff'], eng.grid['logg'], flux)
    eng.ctx.split_components(3)
    with pytest.raises(_lib.MsxError, match='split already'):
        eng.ctx.split_components(2)
    with pytest.raises(ValueError, match='nspec'):       # a binary on three copies
        _stage(eng, c)
    with pytest.raises(ValueError, match='comp'):
        eng.ctx.read_node_component(3, 0, 0)
    with pytest.raises(ValueError, match='comp'):
        eng.ctx.rot_broaden_grid_component(-1, 1000, 500, 50.0, 0.5)
    with pytest.raises(ValueError, match='vsini'):
        eng.ctx.rot_broaden_grid_component(1, 1000, 500, -50.0, 0.5)
    with pytest.raises(ValueError, match='limb'):
        eng.ctx.rot_broaden_grid_component(1, 1000, 500, 50.0, 1.5)
    with pytest.raises(ValueError, match='one value per star'):
        eng.broaden_grid_window([6000.0, 7000.0], 1700, vsini=(10.0, 20.0), limb=(0.1, 0.2, 0.3))
    # the in-path form reads one raw window: refused on a component grid, by the error class of the path
    a, b = golden_engines('B')
    b.ctx.set_path(_lib.PATH_INPATH)
    try:
        with pytest.raises(_lib.MsxError, match='copy per component'):
            b.logposterior(c.theta[:4])
    finally:
        b.ctx.set_path(_lib.PATH_AUTO)
    assert np.array_equal(b.logposterior(c.theta[:4]), a.logposterior(c.theta[:4]))
