"""GPU: rotational broadening (rot_broaden_kernel; DESIGN.md "Rotational broadening") against the NumPy restatement
(tests/rotbroad_numpy.py) -- one spectrum, the drop-in ``broaden``, the staged grid and everything evaluated on it,
and the loader's cache."""
import numpy as np
import pytest

import common
from common import rel_err
import rotbroad_numpy as rb

pytestmark = pytest.mark.gpu

TIGHT = 1e-9


def ctx():
    from mcmc_spec_amd import _lib
    if 'rot_ctx' not in common._cache:
        common._cache['rot_ctx'] = _lib.Context(0)
    return common._cache['rot_ctx']


def spectrum(n, lo, seed):
    rng = np.random.default_rng(seed)
    wl = np.arange(n) * 0.2 + lo
    flux = 1.0 - 0.6 * rng.random(n) ** 6
    return wl, flux


@pytest.mark.parametrize('lo', [3000.0, 7000.0, 30000.0 - 0.2 * 3000])
def test_single_spectrum_matches_the_restatement(lo):
    c = ctx()
    wl, flux = spectrum(3000, lo, seed=int(lo))
    for vsini in (2.0, 10.0, 50.0, 150.0, 400.0, 1000.0):
        for limb in (0.05, 0.6, 1.0):
            got = c.rot_broaden(wl, flux, vsini, limb)
            want = rb.rot_broad(wl, flux, limb, vsini)
            assert rel_err(got, want).max() <= 1e-12, (lo, vsini, limb)


@pytest.mark.parametrize('n,lo,vsini,limb', [
    (64, 7000.0, 400.0, 0.6),      # binnu = 47
    (64, 30000.0, 1000.0, 0.6),    # binnu = 501 > n
    (20, 9000.0, 5000.0, 0.3),     # binnu = 751 > n: the largest LDS tile
    (20, 9000.0, 10000.0, 0.3),    # binnu = 1502: the halo is too wide for the LDS tile (global read path)
    (300, 7000.0, 5.0, 0.6),       # dlmax < dwl: the identity, up to the rounding of f g / g
    (2, 7000.0, 50.0, 1.0),
])
def test_single_spectrum_short_and_extreme(n, lo, vsini, limb):
    wl, flux = spectrum(n, lo, seed=n)
    got = ctx().rot_broaden(wl, flux, vsini, limb)
    want = rb.rot_broad_literal(wl, flux, limb, vsini)
    assert rel_err(got, want).max() <= 1e-12


def test_single_spectrum_refuses_bad_values():
    from mcmc_spec_amd import _lib
    c = ctx()
    wl, flux = spectrum(100, 7000.0, seed=1)
    for vsini, limb in ((0.0, 0.5), (-5.0, 0.5), (50.0, 1.5), (50.0, -0.1), (np.nan, 0.5), (np.inf, 0.5), (50.0, np.inf)):
        with pytest.raises(ValueError):
            c.rot_broaden(wl, flux, vsini, limb)
    with pytest.raises(ValueError):                                  # uneven axis
        c.rot_broaden(np.r_[wl[:50], wl[50:] + 0.01], flux, 50.0, 0.5)
    with pytest.raises(ValueError):                                  # more than 2^19 samples of halo
        c.rot_broaden(wl, flux, 1e9, 0.5)
    assert not isinstance(_lib.MsxError, ValueError)


def test_drop_in_broaden():
    import mcmc_spec_amd.mft6 as m
    from oracle import mft6_oracle as orc
    m.clear_cache()
    wl, flux = spectrum(6000, 6000.0, seed=7)
    base = m.broaden(wl, flux, 1700)[1]
    for vsini, limb in ((60.0, 0.6), (10.0, 1.0), (400.0, 0.05)):
        w, got = m.broaden(wl, flux, 1700, vsini, limb)
        want = rb.rot_broad(wl, orc.broaden(wl, flux, 1700)[1], limb, vsini)
        assert np.array_equal(w, wl) and rel_err(got, want).max() <= 1e-12
    # the reference's condition: rotation only when vsini != 0 and limb != 0
    for vsini, limb in ((0, 0), (50.0, 0), (0, 0.6), (-5.0, 0)):
        assert np.array_equal(m.broaden(wl, flux, 1700, vsini, limb)[1], base)
    for vsini, limb in ((50.0, 1.5), (-5.0, 0.5), (np.nan, 0.5), (50.0, np.nan), (np.inf, 0.5)):
        with pytest.raises(ValueError):
            m.broaden(wl, flux, 1700, vsini, limb)


def restage(eng, W):
    from mcmc_spec_amd import bands, synth
    bl = bands.make_bands(W['tabs'], *W['vega'])
    eng.stage_problem(W['data'], W['err'], W['fr'], W['r'], W['ctm'], W['ptm'], W['tmi'], W['tma'], W['matrix'], nspec=2,
                      bands=bl, av_table=synth.make_av_table(), tmin=W['tmin'], tmax=W['tmax'], prior=W['prior'])


def rotated(npix, phot, vsini=60.0, limb=0.6):
    """The bench's workload, then its grid staged again (in-path placement: the raw window is kept) and broadened with
    rotation; the problem is staged again on the rotated grid."""
    from bench import build_workload
    from mcmc_spec_amd import _lib, synth
    from mcmc_spec_amd.engine import Engine
    key = ('rotated', npix, phot)
    if key not in common._cache:
        eng = Engine(0)
        W = build_workload(eng, npix, phot, keep_host_grid=True, broaden='in_path')
        eng.stage_grid(W['wl'], W['teffs'], W['loggs'], W['flux'])
        eng.broaden_grid_window(W['win'], W['resolution'], 'in_path', vsini=vsini, limb=limb)
        th = synth.draw_walkers(4, seed=1, tmin=W['tmin'], tmax=W['tmax'])
        with pytest.raises(_lib.MsxError, match='no problem staged'):   # the old problem went with the old grid
            eng.logposterior(th)
        restage(eng, W)
        common._cache[key] = (eng, W)
    return common._cache[key]


def test_grid_window_and_logposterior_match_the_oracle():
    from mcmc_spec_amd import synth
    from oracle import mft6_oracle as orc
    eng, W = rotated(4096, False)
    wl = W['wl']
    inside = (wl >= min(W['win'])) & (wl <= max(W['win']))
    specs = synth.grid_to_specs(W['teffs'], W['loggs'], wl, W['flux'])
    specs = orc.broaden_specs_window(specs, W['win'], W['resolution'])
    for it, t in enumerate(W['teffs']):
        for ig, g in enumerate(W['loggs']):
            k = '{}, {}'.format(int(t), float(g))
            specs[k][inside] = rb.rot_broad(wl[inside], specs[k][inside], 0.6, 60.0)
            node = eng.ctx.read_node(it, ig)
            assert np.array_equal(node[~inside], W['flux'][it, ig][~inside]), k      # the wings are untouched
            assert rel_err(node[inside], specs[k][inside]).max() <= 1e-12, k
    th = synth.draw_walkers(64, seed=11, tmin=W['tmin'], tmax=W['tmax'])
    got = eng.logposterior(th)
    edges, mu, sig = synth.make_av_table()

    def avp(d):
        b = int(np.clip(np.searchsorted(edges, d, side='right') - 1, 0, len(mu) - 1))
        return mu[b], sig[b]

    bl = orc.make_band_library(W['tabs'], *W['vega'])
    want = np.array([orc.logposterior(list(t), W['fr'], 2, W['data'], W['err'], W['r'], specs, W['ctm'], W['ptm'],
                                      W['tmi'], W['tma'], W['tmin'], W['tmax'], W['matrix'], avp, prior=W['prior'],
                                      bandlib=bl) for t in th])
    assert np.array_equal(np.isfinite(got), np.isfinite(want)) and np.isfinite(want).sum() > 48
    fin = np.isfinite(want)
    assert rel_err(got[fin], want[fin]).max() < TIGHT


def forms(eng, paths, th):
    from mcmc_spec_amd import _lib
    out = []
    for p in paths:
        eng.ctx.set_path(p)
        out.append(eng.logposterior(th))
    eng.ctx.set_path(_lib.PATH_AUTO)
    return out


def test_forms_agree_bit_for_bit_on_the_rotated_grid():
    from mcmc_spec_amd import _lib, synth
    eng, W = rotated(4096, False)
    th = synth.draw_walkers(2305, seed=9, tmin=W['tmin'], tmax=W['tmax'])
    fused, pair = forms(eng, (_lib.PATH_FUSED, _lib.PATH_PAIR), th)
    assert np.array_equal(fused, pair, equal_nan=True) and np.isfinite(fused).sum() > 2000
    # the per-walker form applies the Gaussian only: refused on a rotated grid, with the rotation named
    eng.ctx.set_path(_lib.PATH_INPATH)
    with pytest.raises(_lib.MsxError, match='rotation'):
        eng.logposterior(th[:8])
    eng.ctx.set_path(_lib.PATH_AUTO)
    assert np.array_equal(eng.logposterior(th[:8]), fused[:8], equal_nan=True)


def test_linked_form_agrees_bit_for_bit_on_the_rotated_grid():
    from mcmc_spec_amd import _lib, synth
    eng, W = rotated(16384, True)
    for n in (5, 128):
        th = synth.draw_walkers(n, seed=40 + n, tmin=W['tmin'], tmax=W['tmax'])
        fused, linked = forms(eng, (_lib.PATH_FUSED, _lib.PATH_LINKED), th)
        assert np.array_equal(fused, linked, equal_nan=True) and np.isfinite(fused).sum() > n // 2


def test_loader_cache_separates_rotated_and_unrotated_grids(tmp_path):
    from mcmc_spec_amd import loader, synth
    import mcmc_spec_amd.mft6 as m
    gdir = synth.write_btsettl_text_grid(str(tmp_path / 'BT-Settl_M-0.0a+0.0'), seed=21)
    args = ([6000.0, 8000.0], [3000, 3200], [4, 5.5], [5000, 9000])
    cache = str(tmp_path / 'grid_cache.npz')
    m.clear_cache()
    plain = loader.spec_interpolator(*args, resolution=1700, grid_dir=gdir)         # today's output, no cache
    rot = loader.spec_interpolator(*args, resolution=1700, grid_dir=gdir, cache=cache, vsini=60, limb=0.6)
    again = loader.spec_interpolator(*args, resolution=1700, grid_dir=gdir, cache=cache, vsini=0)
    keys = [k for k in plain if k != 'wl']
    assert all(np.array_equal(again[k], plain[k]) for k in plain)
    wl = plain['wl']
    inside = (wl >= 6000.0) & (wl <= 8000.0)
    for k in keys:
        assert not np.array_equal(rot[k], plain[k])
        assert np.array_equal(rot[k][~inside], plain[k][~inside])
        assert rel_err(rot[k][inside], rb.rot_broad(wl[inside], plain[k][inside], 0.6, 60.0)).max() <= 1e-12
    # and the cache written by the unrotated call is not served to a rotated request either
    rot2 = loader.spec_interpolator(*args, resolution=1700, grid_dir=gdir, cache=cache, vsini=60, limb=0.6)
    assert all(np.array_equal(rot2[k], rot[k]) for k in rot)
    m.clear_cache()
