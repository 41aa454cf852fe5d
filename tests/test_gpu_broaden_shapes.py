"""GPU: the two implementations of the Gaussian instrumental broadening at the shapes where a tiled LDS
convolution goes wrong -- tile seams, the halo at both ends of the row, even tap counts, the last partial tile, kernels
longer than the tile and than the row, the LDS opt-in and its refusal, and the clamps of the two edge patches.

* the staging placement (``broaden_conv_kernel`` / ``broaden_patch_kernel`` through ``msx_broaden`` and
  ``msx_broaden_grid``) sample by sample against the long-double twin of tests/broaden_numpy.py, inside its derived bound
  ``(lx + 16) 2^-53 sum_k |e_k y|`` (tests/test_broaden_restatement.py shows that four subtly wrong kernels fail it);
* the in-path form (``inpath_conv_kernel`` / ``inpath_resample_kernel``) on small windows of golden case B's grid whose
  pixels read both edge patches: against the fused form on the same staged problem (1e-11, tests/test_gpu_inpath.py) and
  the oracle's restatement of the placement (1e-9), log-likelihood and chi^2;
* ``resample_kernel`` of the same loader path against ``scipy.interpolate.interp1d``, bit for bit.

Every case prints its lx and its worst error / bound (direct) or worst relative deviation (in-path)."""
import numpy as np
import pytest

import common
import broaden_numpy as bn
from common import golden_case, rel_err

pytestmark = pytest.mark.gpu

TIGHT = 1e-9          # tests/test_gpu_parity.py, tests/test_gpu_inpath.py: against the oracle
INPATH_TOL = 1e-11    # tests/test_gpu_inpath.py: the in-path form against the staging placement


@pytest.fixture(scope='module')
def ctx():
    from mcmc_spec_amd._lib import Context
    return Context(0)


# ---- msx_broaden ---------------------------------------------------------------------------------------------------------
def _direct(ctx, n, resolution, maxsig, tag):
    dx, sigma, lx = bn.params(n, resolution, maxsig)
    wl, y, yz = bn.rows(n)
    worst, outs = 0.0, []
    for row in (y, yz):
        got = ctx.broaden(wl, row, resolution, maxsig)
        worst = max(worst, bn.check(got, row, dx, sigma, lx, patched=True))
        outs.append(got)
    print('%s: n %d lx %d LDS %d bytes: worst error / bound %.4f' % (tag, n, lx, bn.lds_bytes(lx), worst))
    return lx, outs


@pytest.mark.parametrize('case', bn.CASES, ids=[c[0] for c in bn.CASES])
def test_broaden_against_the_definition(ctx, case):
    cid, n, resolution, maxsig, _ = case
    assert bn.case_params(case)[0] == n          # (asserts the class of lx the case is there for)
    lx, outs = _direct(ctx, n, resolution, maxsig, cid)
    if lx == 1:                                  # identity: one tap, e / e = 1
        wl, y, yz = bn.rows(n)
        for got, row in zip(outs, (y, yz)):
            assert np.array_equal(got[5:n - 10], row[5:n - 10])


def test_longest_kernel_and_the_refusal_beyond_it(ctx):
    """lx in [8900, 9088]: the largest tile launch_conv accepts (150 KiB of LDS); one tap more is refused before any
    launch (MSX_ERR_RANGE, which the binding raises as ValueError like every range error), and the context goes on to
    give the first cases' bits."""
    firsts = [bn.CASES[0], bn.CASES[5]]          # the identity and the first case with a tile's worth of taps
    rows = [bn.rows(f[1])[:2] for f in firsts]
    before = [ctx.broaden(wl, y, f[2], f[3]) for f, (wl, y) in zip(firsts, rows)]

    def same_bits_as_before():
        return all(np.array_equal(ctx.broaden(wl, y, f[2], f[3]), b) for f, (wl, y), b in zip(firsts, rows, before))

    r_ok, r_no = bn.longest_resolution(), bn.refused_resolution()
    lx, _ = _direct(ctx, bn.N_LONGEST, r_ok, 5.0, 'longest')
    assert 8900 <= lx <= bn.MAX_LX and bn.lds_bytes(lx) <= 150 * 1024
    lx_no = bn.params(bn.N_LONGEST, r_no, 5.0)[2]
    assert lx_no > bn.MAX_LX and bn.lds_bytes(lx_no) > 150 * 1024
    wl2, y2, _ = bn.rows(bn.N_LONGEST)
    with pytest.raises(ValueError, match='kernel too long'):
        ctx.broaden(wl2, y2, r_no, 5.0)
    assert same_bits_as_before()
    # ... as after a kernel that needed the attribute, once the limit has been raised further
    _direct(ctx, bn.CASES[-1][1], bn.CASES[-1][2], bn.CASES[-1][3], 'lds_attribute again')
    assert same_bits_as_before()


def test_broaden_refuses_an_uneven_axis_and_a_short_row(ctx):
    from mcmc_spec_amd import _lib
    wl, y, _ = bn.rows(64)
    bent = wl.copy()
    bent[40:] += 1e-4                            # one step of 0.2001 among 0.2: 5e-4 of the mean step, the limit is 1e-6
    with pytest.raises(ValueError, match='not equidistant'):
        ctx.broaden(bent, y, 1700.0)
    with pytest.raises(_lib.MsxError):
        ctx.broaden(wl[:15], y[:15], 1700.0)
    assert bn.check(ctx.broaden(wl[:16], y[:16], 1700.0), y[:16], *bn.params(16, 1700.0, 5.0), patched=True) <= 1.0


# ---- msx_broaden_grid ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def engine():
    from mcmc_spec_amd.engine import Engine
    return Engine(0)


def _grid_params(wl, i0, n, resolution, maxsig=5.0):
    w = wl[i0:i0 + n]
    m = bn.mean_sequential(w)
    return w[1] - w[0], bn.sigma_of(m, resolution), bn.lx_of(m, w[1] - w[0], resolution, maxsig)


@pytest.mark.parametrize('where', ['left_edge', 'right_edge', 'inside'])
def test_broaden_grid_windows(engine, where):
    c = golden_case('B')
    nwl = len(c.wl)
    i0, n = {'left_edge': (0, 1025), 'right_edge': (nwl - 1027, 1027), 'inside': (2996, 1024)}[where]
    resolution = 1700.0
    engine.stage_specs(c.specs)                  # (the broadening is in place: a fresh copy of the raw grid per window)
    engine.ctx.set_broadening('staging')
    engine.ctx.broaden_grid(i0, n, resolution, 5.0)
    dx, sigma, lx = _grid_params(c.wl, i0, n, resolution)
    nt, ng = len(c.teffs), len(c.loggs)
    worst = 0.0
    for it in range(nt):
        for ig in range(ng):
            got = engine.ctx.read_node_component(0, it, ig)
            raw = c.flux[it, ig]
            assert np.array_equal(got[:i0], raw[:i0]) and np.array_equal(got[i0 + n:], raw[i0 + n:]), (it, ig)
            assert not np.array_equal(got[i0:i0 + n], raw[i0:i0 + n])
            if (it, ig) in ((0, 0), (nt - 1, ng - 1)):
                worst = max(worst, bn.check(got[i0:i0 + n], raw[i0:i0 + n], dx, sigma, lx, patched=True))
                # the same kernel with another stride
                assert np.array_equal(engine.ctx.broaden(c.wl[i0:i0 + n], raw[i0:i0 + n], resolution, 5.0), got[i0:i0 + n])
    print('broaden_grid %s: window (%d, %d) lx %d: worst error / bound %.4f' % (where, i0, n, lx, worst))


# ---- msx_resample_linear -------------------------------------------------------------------------------------------------
def test_resample_linear_is_interp1d_bit_for_bit(ctx):
    from scipy.interpolate import interp1d
    xs, ys, xq = bn.resample_inputs()
    want = interp1d(xs, ys)(xq)
    assert np.array_equal(bn.resample_numpy(xs, ys, xq), want)
    got = ctx.resample_linear(xs, ys, xq)
    assert np.array_equal(got, want), np.flatnonzero(got != want)[:8]
    for m in (255, 256, 257):                    # each side of one workgroup of queries
        assert np.array_equal(ctx.resample_linear(xs, ys, xq[-m:]), want[-m:])
    x2, y2 = np.array([1.0, 2.5]), np.array([0.3, -1.7])
    q2 = np.concatenate([[1.0, 2.5], np.random.default_rng(1).uniform(1.0, 2.5, size=50)])
    assert np.array_equal(ctx.resample_linear(x2, y2, q2), interp1d(x2, y2)(q2))


# ---- the in-path form at small shapes ------------------------------------------------------------------------------------
NPROBE = 16
PICK = [0, 1, 2, 5, 6, 7]     # the walkers the oracle restates (tests/test_gpu_inpath.py)


def PATCH_SAMPLES(n):
    """lower model samples whose pixels read the patches and their clamps"""
    return (0, 4, 5, n - 12, n - 11, n - 2)


def _walkers(c):
    from mcmc_spec_amd import synth
    th = synth.draw_walkers(NPROBE, seed=11, tmin=c.tmin, tmax=c.tmax)
    th[1, 2] = 0.0          # unreddened
    th[2, 0] = 3800.0       # on a Teff node
    th[3, 3] = 0.04         # rejected by the prior box
    th[4, 1] = 2000.0       # outside the isochrone: ValueError status
    return th


def _window_data(c, i0, n, npix):
    """npix pixels inside grid samples [i0, i0 + n): the recipe of variant_cases.synthetic_data restricted to the window,
    six of them 0.05 A above window samples 0, 4, 5, n - 12, n - 11 and n - 2.  (data, err, r, w_aa)."""
    rng = np.random.default_rng(7000 + 10 * n + npix)
    wl = c.wl[i0:i0 + n]
    special = np.array([wl[a] + 0.05 for a in PATCH_SAMPLES(n)])
    aa = np.sort(np.concatenate([special, rng.uniform(wl[0] + 0.05, wl[n - 2] + 0.05, size=npix - len(special))]))
    um = aa / 1e4
    lo = np.searchsorted(wl, um * 1e4, side='right') - 1
    assert lo.min() == 0 and lo.max() == n - 2 and set(PATCH_SAMPLES(n)) <= set(lo.tolist())
    data = [um, 1.0 + 0.1 * rng.normal(size=npix)]
    err = rng.uniform(0.01, 0.2, size=npix)
    return data, err, [um.min(), um.max()], [float(wl[0]) - 0.05, float(wl[-1]) + 0.05]


def _stage(engine, c, i0, n, npix, resolution):
    from mcmc_spec_amd import bands
    data, err, r, w = _window_data(c, i0, n, npix)
    engine.stage_specs(c.specs)
    engine.broaden_grid_window(w, resolution, 'in_path')
    engine.stage_problem(data, err, c.fr, r, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=2, bands=bands.make_bands(c.tables, *c.vega),
                         av_table=common.av_table_exact(), tmin=c.tmin, tmax=c.tmax, prior=c.prior)
    return data, err, r, w


def _both_forms(engine, th):
    """{mode: (in-path values, statuses, fused values, statuses)} on the staged problem."""
    from mcmc_spec_amd import _lib
    out = {}
    for mode in ('LOGLIKE', 'CHISQ', 'LOGPOST'):
        m = getattr(_lib, 'MODE_' + mode)
        engine.ctx.set_path(_lib.PATH_FUSED)
        ref, st_ref = engine.ctx.logprob_batch(th, m)
        assert engine.ctx.last_form() == _lib.FORM_FUSED
        engine.ctx.set_path(_lib.PATH_INPATH)
        got, st = engine.ctx.logprob_batch(th, m)
        assert engine.ctx.last_form() == _lib.FORM_INPATH
        out[mode] = (got, st, ref, st_ref)
    return out


def _check_inpath(tag, engine, c, i0, n, npix, resolution, staged, lx):
    from mcmc_spec_amd import _lib
    from oracle import mft6_oracle as orc
    data, err, r, w = staged
    th = _walkers(c)
    res = _both_forms(engine, th)
    worst = 0.0
    for mode, (got, st, ref, st_ref) in res.items():
        assert np.array_equal(st, st_ref), (tag, mode, st, st_ref)
        assert np.array_equal(np.isfinite(got), np.isfinite(ref)), (tag, mode)
        fin = np.isfinite(ref)
        if mode == 'LOGPOST':
            assert np.isneginf(got[3]) and fin.sum() == NPROBE - 2
        else:
            assert st[4] == _lib.W_VALUEERROR and fin[3]
        e = rel_err(got[fin], ref[fin]).max()
        print('%s: window (%d, %d) npix %d lx %d %s: in-path against the staging placement %.3e' % (tag, i0, n, npix, lx, mode, e))
        assert e < INPATH_TOL, (tag, mode, e)
        worst = max(worst, e)
    if lx <= n:   # (a kernel longer than the window: np.convolve returns lx samples and the oracle cannot restate it)
        specs = orc.broaden_specs_window(c.specs, w, resolution)
        kw = dict(bandlib=c.bandlib, inpath=dict(specs_raw=c.specs, w=w, resolution=resolution))
        want = np.array([orc.loglikelihood(list(th[k]), c.fr, 2, data, err, r, specs, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, **kw)
                         for k in PICK])
        e_ll = rel_err(res['LOGLIKE'][0][PICK], want).max()
        e_chi = rel_err(res['CHISQ'][0][PICK], -2.0 * want).max()
        print('%s: lx %d: in-path against the oracle: log-likelihood %.3e, chi^2 %.3e' % (tag, lx, e_ll, e_chi))
        assert e_ll < TIGHT and e_chi < TIGHT, (tag, e_ll, e_chi)
    return worst


def _even_resolution(c, i0, n):
    r = 1700.0
    while _grid_params(c.wl, i0, n, r)[2] % 2:
        r *= 0.999
    return r


I0 = 5000    # 6000 A: inside golden case B's data range
INPATH_CASES = {
    # id: (first grid sample, window samples, pixels, resolution or None = the first below 1700 that gives an even lx)
    'n1024': (I0, 1024, 40, 1700.0),
    'n1025': (I0, 1025, 63, 1700.0),
    'n1026': (I0, 1026, 64, 5000.0),
    'n1027': (I0, 1027, 65, 400.0),
    'n2049': (I0, 2049, 257, 1700.0),
    'n300': (I0, 300, 40, 1700.0),
    'n300_longer_than_the_window': (I0, 300, 40, 400.0),
    'n3000_long': (I0, 3000, 300, 60.0),
    'even_lx': (I0, 1030, 70, None),
    'grid_left_edge': (0, 1025, 63, 1700.0),
    'grid_right_edge': (-1027, 1027, 65, 1700.0),
}


@pytest.mark.parametrize('cid', list(INPATH_CASES))
def test_inpath_at_small_shapes(engine, cid):
    c = golden_case('B')
    i0, n, npix, resolution = INPATH_CASES[cid]
    i0 = i0 if i0 >= 0 else len(c.wl) + i0
    if resolution is None:
        resolution = _even_resolution(c, i0, n)
    lx = _grid_params(c.wl, i0, n, resolution)[2]
    if cid == 'even_lx':
        assert lx % 2 == 0
    if cid == 'n3000_long':
        assert lx > bn.TILE and bn.inpath_lds_bytes(lx) > 48 * 1024
    if cid == 'n300_longer_than_the_window':
        assert lx > n
    if cid == 'grid_right_edge':
        assert i0 + n == len(c.wl)
    staged = _stage(engine, c, i0, n, npix, resolution)
    _check_inpath(cid, engine, c, i0, n, npix, resolution, staged, lx)


def test_inpath_sub_batches_at_small_cost(engine, monkeypatch):
    """MSX_INPATH_MB=1 at stage_problem: about 80 walkers of the (1027, 65) problem fit the form's scratch, so 300 walkers
    cross three sub-batch boundaries.  A walker's value is its own."""
    from mcmc_spec_amd import _lib
    c = golden_case('B')
    i0, n, npix, resolution = INPATH_CASES['n1027']
    monkeypatch.setenv('MSX_INPATH_MB', '1')
    _stage(engine, c, i0, n, npix, resolution)
    monkeypatch.delenv('MSX_INPATH_MB')
    engine.ctx.set_path(_lib.PATH_INPATH)
    rows = engine.ctx.launch_info(300)['walkers_per_sub_batch']
    assert 16 <= rows < 100, rows
    probes = _walkers(c)
    idx = np.arange(300) % NPROBE
    big = probes[idx]
    a, st = engine.ctx.logprob_batch(big, _lib.MODE_LOGLIKE)
    assert engine.ctx.last_form() == _lib.FORM_INPATH
    alone, st_alone = engine.ctx.logprob_batch(probes, _lib.MODE_LOGLIKE)
    assert np.array_equal(a, alone[idx], equal_nan=True) and np.array_equal(st, st_alone[idx])
    perm = np.random.default_rng(0).permutation(300)
    b, stb = engine.ctx.logprob_batch(big[perm], _lib.MODE_LOGLIKE)
    assert np.array_equal(b, a[perm], equal_nan=True) and np.array_equal(stb, st[perm])
    seven, _ = engine.ctx.logprob_batch(big[:7], _lib.MODE_LOGLIKE)
    assert np.array_equal(seven, a[:7], equal_nan=True)
    print('sub-batches: %d walkers per sub-batch, 300 walkers, %d finite' % (rows, int(np.isfinite(a).sum())))
