"""GPU: derived posteriors (include/msx.h, msx_stage_products / msx_products_batch / msx_series_derive;
mcmc_spec_amd.products; the device samplers' get_products) against the reference's own
make_composite(plot=True) run (tests/golden/golden_products.npz) and against the NumPy twin (tests/products_numpy.py).

Bars: the project's bar for reference goldens, 1e-9 (README) -- relative for fluxes and factors, absolute for magnitudes
and log g (a contrast may be 0).  Derived rows against msx_products_batch, and summaries of a derived series against
NumPy on the values read back, are compared exactly."""
import numpy as np
import pytest

import common
import products_numpy as pn
from common import golden_case

pytestmark = pytest.mark.gpu

TOL = 1e-9
BIN_COLS = ['kep_pri', 'kep_sec', 'gaia_pri', 'gaia_sec', 'gaia_sum', 'kep_contrast', 'pri_corr', 'sec_corr', 'logg:0', 'logg:1',
            'mass:0', 'mass:1', 'lum:0', 'lum:1']
TRI_COLS = ['kep_pri', 'kep_sec', 'kep_ter', 'logg:0', 'logg:1', 'logg:2', 'mass:0', 'mass:1', 'mass:2', 'lum:0', 'lum:1', 'lum:2']
CASES = {'bin': ('B', True), 'nod': ('A', False), 'tri': ('C', True)}


def goldens():
    if 'products_g' not in common._cache:
        common._cache['products_g'] = dict(np.load(pn.GOLDEN))
    return common._cache['products_g']


def gaia_band(g):
    from mcmc_spec_amd import bands
    b = bands.Band('Gaia_G', g['gaia_wl'], g['gaia_tm'], float(g['gaia_zero_flux'][0]))
    b.zero_mag = float(g['gaia_zero_mag'][0])
    return b


def stage_products(eng, g):
    eng.stage_products((g['kepler_wl'], g['kepler_tm']), gaia=gaia_band(g), matrix=pn.products_matrix())
    return eng


def engine(which, dist_fit=True, specs=None, products=True, prepare=None):
    """Golden case `which` on the isochrone of the product goldens (tests/products_numpy.py), products staged."""
    from mcmc_spec_amd import bands
    from mcmc_spec_amd.engine import Engine
    key = ('products_eng', which, dist_fit, products)
    if specs is None and prepare is None and key in common._cache:
        return common._cache[key]
    c = golden_case(which)
    eng = Engine(0)
    eng.stage_specs(c.specs if specs is None else specs)
    if prepare is not None:
        prepare(eng)
    eng.stage_problem(c.data, c.err, c.fr, c.r, c.ctm, c.ptm, c.tmi, c.tma, pn.products_matrix(), nspec=c.nspec,
                      bands=bands.make_bands(c.tables, *c.vega), av_table=common.av_table_exact(), tmin=c.tmin, tmax=c.tmax,
                      prior=0, dist_fit=dist_fit, rad_prior=True)
    if products:
        stage_products(eng, goldens())
    if specs is None and prepare is None:
        common._cache[key] = eng
    return eng


def close(got, want, absolute, what):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, what
    d = np.abs(got - want) if absolute else np.abs(got - want) / np.abs(want)
    print('{}: worst {} difference {:.3e}'.format(what, 'absolute' if absolute else 'relative', float(np.max(d))))
    assert np.all(d <= TOL), (what, float(np.nanmax(d)))


def expected_columns(ref, nspec):
    """The goldens' (or the twin's) arrays in the order of BIN_COLS / TRI_COLS, and which of those are compared absolutely."""
    if nspec == 2:
        cols = [ref['mags'][:, k] for k in range(5)] + [ref['dkep'], ref['pri_corr'], ref['sec_corr']]
        absolute = [True] * 6 + [False, False]
    else:
        # the device keeps -2.5 log10 of the plain sum; the division by the zp list stays in Python (mft6.py:820-825)
        cols = [ref['mags'][:, s, 0] - 2.5 * np.log10(pn.ZP[0]) for s in range(3)]
        absolute = [True] * 3
    for name in ('logg', 'mass', 'lum'):
        cols += [ref[name][:, s] for s in range(nspec)]
        absolute += [name == 'logg'] * nspec
    return np.stack(cols, axis=1), absolute


def check_case(tag, theta, got, ref, what):
    want, absolute = expected_columns(ref, golden_case(CASES[tag][0]).nspec)
    for j, a in enumerate(absolute):
        close(got[:, j], want[:, j], a, '{} {} column {}'.format(what, tag, j))


@pytest.mark.parametrize('tag', sorted(CASES))
def test_batch_against_the_references_run_and_the_twin(tag):
    from mcmc_spec_amd import products
    g = goldens()
    which, dist = CASES[tag]
    c = golden_case(which)
    eng = engine(which, dist_fit=dist)
    theta = g[tag + '_theta']
    cols = BIN_COLS if c.nspec == 2 else TRI_COLS
    got, status = products.evaluate(eng, theta, cols, with_status=True)
    assert np.all(status == 0)
    check_case(tag, theta, got, {k[len(tag) + 1:]: v for k, v in g.items() if k.startswith(tag + '_')}, 'goldens')
    check_case(tag, theta, got, pn.evaluate(c, theta, dist, g), 'twin')
    if c.nspec == 3:  # the six-element arrays of the reference's tuple: the device's magnitude and the zp list
        for s in range(3):
            close(got[:, s, None] + 2.5 * np.log10(np.array(pn.ZP))[None, :], g['tri_mags'][:, s, :], True, 'triple / zp, star {}'.format(s))


@pytest.mark.parametrize('n', [1, 63, 64, 65, 257])
def test_batch_sizes(n):
    """One short of, at and one past a wave; more than one workgroup: sample i of a batch has the bits it has alone."""
    from mcmc_spec_amd import products
    g = goldens()
    eng = engine('B')
    base = g['bin_theta']
    theta = base[np.arange(n) % len(base)].copy()
    theta[:, 0] += 0.37 * (np.arange(n) // len(base))   # (no two rows alike)
    got = products.evaluate(eng, theta, BIN_COLS)
    assert got.shape == (n, len(BIN_COLS)) and np.all(np.isfinite(got))
    for i in sorted({0, n // 2, n - 1}):
        assert np.array_equal(products.evaluate(eng, theta[i], BIN_COLS), got[i]), i
    m = min(n, len(base))
    check_case('bin', theta[:m], got[:m], {k[4:]: v[:m] for k, v in g.items() if k.startswith('bin_')}, 'goldens, n = {}'.format(n))


def test_model_contrast_and_photometry_columns():
    """CONTRAST(f) / PHOT(p): the staged problem's band terms, as make_composite(plot=False) returns them (mft6.py:741,
    :780-783)."""
    from mcmc_spec_amd import products
    from oracle import mft6_oracle as orc
    g = goldens()
    for which, nc, nph in (('B', 2, 6), ('C', 4, 6)):
        c = golden_case(which)
        eng = engine(which)
        theta = g['bin_theta'] if c.nspec == 2 else g['tri_theta']
        got = products.evaluate(eng, theta, ['contrast:{}'.format(f) for f in range(nc)] + ['phot:{}'.format(p) for p in range(nph)])
        want = []
        for p in theta:
            tt, rad, dist = pn.sample_args(c, p, True)
            lg = [float(orc.get_logg(t, pn.products_matrix())) for t in tt]
            _, _, con, _, ph, _ = orc.make_composite(tt, lg, rad, dist, c.fr[2], c.fr[5], c.r, c.specs, c.ctm, c.ptm, c.tmi, c.tma,
                                                     nspec=c.nspec, bandlib=c.bandlib)
            want.append(list(con) + list(ph))
        close(got, np.array(want, dtype=float), True, 'contrast / phot, case ' + which)


def test_component_grid_reads_each_stars_copy():
    """A component grid with two different v sin i: star s's integrals come from copy s (node_stride)."""
    from mcmc_spec_amd import products
    g = goldens()
    c = golden_case('B')
    eng = engine('B', prepare=lambda e: e.broaden_grid_window([6000.0, 8000.0], 1700, vsini=(6.0, 30.0), limb=(0.4, 0.6)))
    assert eng.ctx.lib is not None
    specs = []
    for comp in range(2):
        d = {'wl': c.wl}
        for it, t in enumerate(c.teffs):
            for ig, lg in enumerate(c.loggs):
                d['{}, {}'.format(int(t), float(lg))] = eng.ctx.read_node_component(comp, it, ig)
        specs.append(d)
    assert not np.array_equal(specs[0]['3800, 4.5'], specs[1]['3800, 4.5'])
    theta = g['bin_theta'][:5]
    got = products.evaluate(eng, theta, ['kep_pri', 'kep_sec', 'kep_contrast'])
    want = []
    for p in theta:
        tt, rad, dist = pn.sample_args(c, p, True)
        from oracle import mft6_oracle as orc
        lg = [float(orc.get_logg(t, pn.products_matrix())) for t in tt]
        k = []
        for s in range(2):
            w, _, stars = pn.composite_plot(c, tt, lg, rad, dist, g['kepler_wl'], specs=specs[s])
            k.append(pn.kepler_integrals(w, [stars[s]], g['kepler_wl'], g['kepler_tm'], 'trapz')[0])
        m = -2.5 * np.log10(np.array(k))
        want.append([m[0], m[1], m[1] - m[0]])
    close(got, np.array(want), True, 'component grid')
    one = products.evaluate(engine('B'), theta, ['kep_sec'])
    assert not np.array_equal(one[:, 0], got[:, 1])
    eng.ctx.close()


def test_a_teff_outside_the_product_isochrone():
    """The product isochrone ends at its 200th row (6,171 K here), the problem's at 6,500 K: with a MASS or LUM column a
    Teff between them is the ValueError interp1d raises (mft6.py:2685); its neighbours are untouched."""
    from mcmc_spec_amd import _lib, products
    g = goldens()
    eng = engine('B')
    theta = g['bin_theta'][:5].copy()
    alone = products.evaluate(eng, theta, BIN_COLS)
    bad = theta.copy()
    bad[2, 1] = 6300.0
    got, status = products.evaluate(eng, bad, BIN_COLS, with_status=True)
    assert list(status) == [0, 0, _lib.W_VALUEERROR, 0, 0]
    assert np.all(np.isnan(got[2])) and np.array_equal(got[[0, 1, 3, 4]], alone[[0, 1, 3, 4]])
    # without such a column the isochrone that counts is the problem's: the bracket then runs past the last grid node
    got, status = products.evaluate(eng, bad, ['kep_contrast'], with_status=True)
    assert list(status) == [0, 0, _lib.W_INDEXERROR, 0, 0] and np.isnan(got[2, 0])
    bad[2, 1] = 6600.0
    assert products.evaluate(eng, bad, ['kep_contrast'], with_status=True)[1][2] == _lib.W_VALUEERROR
    bad[2, 1] = np.nan
    assert products.evaluate(eng, bad, ['kep_contrast'], with_status=True)[1][2] == _lib.W_REJECT


def test_refusals():
    from mcmc_spec_amd import _lib, products
    eng = engine('B')
    th = goldens()['bin_theta'][:2]
    for cols in (['kep_ter'], ['contrast:2'], ['phot:6'], ['logg:2'], ['coord:6'], [_lib.pcol_bandmag(2, 0)], [0x0b000000],
                 list(range(6)) * 11):
        with pytest.raises(ValueError):
            products.evaluate(eng, th, np.array(cols) if not isinstance(cols[0], str) else cols)
    bare = engine('B', products=False)
    with pytest.raises(_lib.MsxError) as e:
        products.evaluate(bare, th, ['kep_contrast'])
    assert e.value.code == _lib.MSX_ERR_STATE
    assert np.array_equal(products.evaluate(eng, th, ['coord:3'])[:, 0], th[:, 3])


def _chain(counts, rows, seed):
    """(rows, sum counts, 6): walkers inside the grid, as a sampler's chain has them."""
    from mcmc_spec_amd import synth
    c = golden_case('B')
    nw = sum(counts)
    th = synth.draw_walkers(rows * nw, seed=seed, tmin=c.tmin, tmax=c.tmax)
    return th.reshape(rows, nw, 6)


NROWS = 300   # past the 256 rows the destination's first growth gives it: a second growth that carries rows over
DERIVE_COLS = ['kep_contrast', 'pri_corr', 'sec_corr', 'gaia_pri', 'mass:1', 'coord:0']


@pytest.mark.parametrize('counts', [(12, 50), (12, 1, 18)])
def test_derive_is_the_batch_row_by_row(counts):
    """Members on different data (golden cases B, A and B without distance); the destination starts with room for 4 rows
    and grows twice (to 256 rows at the 5-row call, to 512 at the 300-row call, which carries 130 rows over); every derived row carries the bits of msx_products_batch on that row; the summaries of the derived series
    are NumPy's on the values read back."""
    from mcmc_spec_amd import _lib, products, summary
    engs = [engine('B'), engine('A'), engine('B', dist_fit=False)][:len(counts)]
    x = _chain(counts, NROWS, 17 + len(counts))
    x[7, 3, 1] = 6300.0   # one sample whose mass look-up fails: NaN in its derived row, status per member
    nw = sum(counts)
    src = _lib.Series(engs[0].ctx, nw, 6, counts)
    src.append(x)
    codes = products.columns(DERIVE_COLS)
    dst = _lib.Series(engs[0].ctx, nw, len(codes), counts, cap_hint=4)
    off = np.concatenate([[0], np.cumsum(counts)])
    want = np.empty((NROWS, nw, len(codes)))
    for m, e in enumerate(engs):
        blk = x[:, off[m]:off[m + 1], :].reshape(-1, 6)
        want[:, off[m]:off[m + 1], :] = products.evaluate(e, blk, codes).reshape(NROWS, counts[m], len(codes))
    for row0, n in ((0, 1), (0, 5), (5, 125), (130, NROWS - 130)):   # 1 row; 5 rows (room for 4 grows to 256); 130; 300 (it grows again)
        worst = src.derive([e.ctx for e in engs], codes, dst, row0, n)
        assert dst.rows == row0 + n
        assert np.array_equal(dst.read(), want[:row0 + n], equal_nan=True), (row0, n)
        assert list(worst) == [_lib.W_VALUEERROR if (row0 <= 7 < row0 + n and m == 0) else 0 for m in range(len(counts))]
    assert np.isnan(want[7, 3]).all() and np.isfinite(np.delete(want.reshape(-1, len(codes)), 7 * nw + 3, axis=0)).all()
    # every existing consumer on the derived series: order statistics, counts, 2-D counts -- NumPy's numbers exactly
    # (the selection rows[10::3] leaves the failed sample's row out: NumPy's quantiles of NaN are another matter)
    got = summary.summary_of(dst, NROWS, (0.16, 0.5, 0.84), None, 10, 3)
    vals = dst.read()[10::3]
    assert np.all(np.isfinite(vals))
    k = len(counts)
    flats = [vals[:, off[m]:off[m + 1], :].reshape(-1, len(codes)) for m in range(k)]
    for m in range(k):
        _same({name: v[m] for name, v in got.items()}, _host_summary(flats[m]))
    lo, hi = got['min'][:, :2], np.nextafter(got['max'][:, :2], np.inf)
    edges = np.stack([[np.linspace(lo[m, j], hi[m, j], 12) for j in range(2)] for m in range(k)])
    h = dst.hist(NROWS, 10, 3, [0, 1], edges)
    h2 = dst.hist2d(NROWS, 10, 3, [(0, 1)], edges[:, :1], edges[:, 1:2])
    for m in range(k):
        for j in range(2):
            assert np.array_equal(h[m, j], np.histogram(flats[m][:, j], bins=edges[m, j])[0]), (m, j)
        want2 = np.histogram2d(flats[m][:, 0], flats[m][:, 1], bins=[edges[m, 0], edges[m, 1]])[0]
        assert np.array_equal(h2[m, 0], want2.astype(np.int64)), m
    # the derived series is a series: its autocorrelation is defined (past the failed sample's row, whose columns are NaN)
    f = dst.acf(NROWS, discard=10, dims=[5])
    assert f.shape[0] == k and np.all(np.isfinite(f[:, 5, :3]))
    src.close()
    dst.close()


def test_derive_refusals():
    from mcmc_spec_amd import _lib, products
    engB, bare = engine('B'), engine('B', products=False)
    x = _chain((4,), 6, 3)
    src = _lib.Series(engB.ctx, 4, 6)
    src.append(x)
    codes = products.columns(['kep_contrast', 'pri_corr'])
    dst = _lib.Series(engB.ctx, 4, 2)
    with pytest.raises(_lib.MsxError) as e:      # a member without staged products
        src.derive([bare.ctx], codes, dst, 0, 6)
    assert e.value.code == _lib.MSX_ERR_STATE and 'member 0' in e.value.msg
    with pytest.raises(ValueError):              # rows past the source
        src.derive([engB.ctx], codes, dst, 0, 7)
    with pytest.raises(ValueError):              # a gap in the destination
        src.derive([engB.ctx], codes, dst, 2, 2)
    with pytest.raises(ValueError):              # a code the member cannot answer
        src.derive([engB.ctx], [_lib.pcol_bandmag(5, 0), 0], dst, 0, 6)
    with pytest.raises(_lib.MsxError):           # the destination's width is not ncols
        src.derive([engB.ctx], codes[:1], dst, 0, 6)
    wide = _lib.Series(engB.ctx, 4, 8)
    with pytest.raises(ValueError):              # more columns than a series is wide
        src.derive([engB.ctx], list(range(6)) + codes + [0], wide, 0, 6)
    src.derive([engB.ctx], codes, dst, 0, 6)     # ... and all of that left both series usable
    assert np.array_equal(dst.read().reshape(-1, 2), products.evaluate(engB, x.reshape(-1, 6), codes))
    for s in (src, dst, wide):
        s.close()


def _host_summary(flat, q=(0.16, 0.5, 0.84)):
    return {'count': flat.shape[0], 'min': flat.min(axis=0), 'max': flat.max(axis=0), 'median': np.median(flat, axis=0),
            'quantiles': np.quantile(flat, q, axis=0).T}


def _same(got, want):
    assert sorted(got) == sorted(want)
    for name in want:
        assert np.array_equal(got[name], want[name]), name


PRODUCT_COLS = ['kep_contrast', 'pri_corr', 'sec_corr']


@pytest.mark.parametrize('mode', ['device', 'host'])
def test_sampler_get_products(mode):
    """16 walkers x 40 iterations: the summary of the derived columns is NumPy's on evaluate(get_chain(flat=True)), from
    the chain on the device or uploaded, with and without a caller's draw of flat samples."""
    from mcmc_spec_amd import products, synth
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    eng = engine('B')
    c = golden_case('B')
    s = DeviceEnsembleSampler(16, 6, eng, seed=5, chunk=7, autocorr=mode)
    s.run_mcmc(synth.draw_walkers(16, seed=9, tmin=c.tmin, tmax=c.tmax), 40)
    flat = s.get_chain(discard=4, thin=3, flat=True)
    vals = products.evaluate(eng, flat, PRODUCT_COLS)
    assert np.all(np.isfinite(vals))
    _same(s.get_products(PRODUCT_COLS, discard=4, thin=3), _host_summary(vals))
    idx = np.random.default_rng(3).choice(len(flat), 100, replace=False)
    _same(s.get_products(PRODUCT_COLS, discard=4, thin=3, indices=idx), _host_summary(vals[idx]))


@pytest.mark.parametrize('mode', ['device', 'host'])
def test_group_sampler_get_products(mode):
    from mcmc_spec_amd import products, synth
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    engs = [engine('B'), engine('A')]
    c = golden_case('B')
    counts = [16, 12]
    grp = TargetGroup(engs)
    dev = DeviceGroupSampler(counts, 6, grp, seeds=[40, 41], chunk=16, autocorr=mode)
    dev.run_mcmc([synth.draw_walkers(counts[k], seed=70 + k, tmin=c.tmin, tmax=c.tmax) for k in range(2)], 40)
    got = dev.get_products(PRODUCT_COLS, discard=4, thin=3)
    idx = np.random.default_rng(4).choice(12 * 12, 50, replace=False)
    drawn = dev.get_products(PRODUCT_COLS, discard=4, thin=3, indices=idx)
    for k in range(2):
        vals = products.evaluate(engs[k], dev.get_chain(k, discard=4, thin=3, flat=True), PRODUCT_COLS)
        _same({name: v[k] for name, v in got.items()}, _host_summary(vals))
        _same({name: v[k] for name, v in drawn.items()}, _host_summary(vals[idx]))
    _same(dev.get_products(PRODUCT_COLS, discard=4, thin=3, k=1), {name: v[1] for name, v in got.items()})
    grp.close()


# ---- spectra of samples on the data pixels (msx_products_spectra) --------------------------------------------------------
def _koi_case():
    """A KOI target of tests/golden/golden_koi.npz (1,194 px) as a case the twin understands."""
    import types
    from test_koi_config5 import koi_cases, koi_problem
    gk, tags = koi_cases()
    data, err, fr, r, ctm, ptm, tmi, tma = koi_problem(gk, tags[0])
    cA = golden_case('A')
    return types.SimpleNamespace(nspec=2, data=data, err=err, fr=fr, r=r, ctm=ctm, ptm=ptm, tmi=tmi, tma=tma, specs=cA.specs,
                                 bandlib=cA.bandlib, tables=cA.tables, vega=cA.vega, tmin=cA.tmin, tmax=cA.tmax)


def _engine_of(c):
    from mcmc_spec_amd import bands
    from mcmc_spec_amd.engine import Engine
    eng = Engine(0)
    eng.stage_specs(c.specs)
    eng.stage_problem(c.data, c.err, c.fr, c.r, c.ctm, c.ptm, c.tmi, c.tma, pn.products_matrix(), nspec=c.nspec,
                      bands=bands.make_bands(c.tables, *c.vega), tmin=c.tmin, tmax=c.tmax)
    return stage_products(eng, goldens())


def _spectra_case(which):
    if which == 'K':
        if 'products_koi' not in common._cache:
            c = _koi_case()
            common._cache['products_koi'] = (c, _engine_of(c))
        return common._cache['products_koi']
    return golden_case(which), engine(which)


def _spectra_theta(which, n=8):
    from mcmc_spec_amd import synth
    c = golden_case('C' if which == 'C' else 'B')
    g = goldens()
    th = np.array(np.vstack([g['tri_theta'], c.theta[6:8]]) if which == 'C' else g['bin_theta'][:n], dtype=float)
    if which != 'C' and len(th) < n:
        th = np.vstack([th, synth.draw_walkers(n - len(th), seed=21, tmin=c.tmin, tmax=c.tmax)])
    return th


@pytest.mark.parametrize('which', ['B', 'A', 'K', 'C'])
def test_spectra_against_goldens_and_twin(which):
    """Cases B (700 px: pad pixels, unordered wavelengths), A (4,154 px), a KOI target (1,194 px) and a triple: every row
    against the twin (and the reference's own arrays where the goldens hold them) to 1e-9; row 0 is the sum of rows 1.. in
    star order, bit for bit; pixel order; the median scale is np.median's; A_V = 0 is no reddening."""
    from mcmc_spec_amd import products
    g = goldens()
    c, eng = _spectra_case(which)
    theta = _spectra_theta(which, 4)
    if which == 'B':
        theta = g['bin_theta'][[0, 2, 5]]            # the goldens' samples; [1] has A_V = 0
    elif which == 'A':
        theta = np.vstack([g['specA_theta'], theta[2:3]])
    raw, one, status = products.spectra(eng, theta, median_scale=False, with_status=True)
    scaled, scale = products.spectra(eng, theta, median_scale=True)
    ns, npix = c.nspec, len(c.data[0])
    assert raw.shape == (len(theta), 1 + ns, npix) and np.all(status == 0) and np.all(one == 1.0)
    for i, p in enumerate(theta):
        total = raw[i, 1] + raw[i, 2] if ns == 2 else raw[i, 1] + raw[i, 2] + raw[i, 3]
        assert np.array_equal(raw[i, 0], total)                                    # the sum in star order, bit for bit
        assert np.array_equal(raw[i, 1:], scaled[i, 1:])
        factor = np.median(c.data[1]) / np.median(raw[i, 0])                       # mft6.py:2409, np.median exactly
        assert scale[i] == factor and np.array_equal(scaled[i, 0], raw[i, 0] * factor)
        want = pn.spectra(c, p, g)                                                 # [comp, stars.., scaled comp], pixel order
        close(raw[i], want[:1 + ns], False, 'spectra {} sample {} vs twin'.format(which, i))
        close(scaled[i, 0], want[-1], False, 'scaled composite {} sample {} vs twin'.format(which, i))
    if which in ('A', 'B'):
        ref = g['spec' + which]
        n = len(ref)
        close(raw[:n], ref[:, :3], False, 'spectra {} vs the reference'.format(which))
        close(scaled[:n, 0], ref[:, 3], False, 'scaled composite {} vs the reference'.format(which))
    if which == 'B':   # A_V = 0 and a negative A_V: no reddening (mft6.py:1161); the unordered pixels come back in their order
        assert theta[1, 2] == 0.0
        neg = theta[1].copy()
        neg[2] = -0.3
        assert np.array_equal(products.spectra(eng, neg, median_scale=False)[0], raw[1])
        assert np.any(np.diff(c.data[0]) < 0)
        order = np.argsort(c.data[0], kind='stable')
        assert not np.array_equal(raw[0, 0], raw[0, 0][order])


@pytest.mark.parametrize('which', ['B', 'A', 'K', 'C'])
def test_spectra_close_the_loop_with_the_hot_path(which):
    """No reference needed: from the emitted unscaled composite the host redoes the median scale, the quadratic fit and
    chi^2 in NumPy, adds the band terms from CONTRAST / PHOT, and must land on msx_logprob_batch(MSX_MODE_LOGLIKE) to 1e-9
    relative, for 8 samples per case."""
    from mcmc_spec_amd import products
    from oracle import mft6_oracle as orc
    c, eng = _spectra_case(which)
    theta = _spectra_theta(which, 8)[:8]
    assert len(theta) == 8
    raw, _ = products.spectra(eng, theta, median_scale=False)
    nc, nph = len(c.fr[2]), len(c.fr[5])
    bands_ = products.evaluate(eng, theta, ['contrast:{}'.format(f) for f in range(nc)] + ['phot:{}'.format(p) for p in range(nph)])
    got = eng.loglikelihood(theta)
    wl, spec = np.asarray(c.data[0]), np.asarray(c.data[1])
    phot_cwl = np.array([float(x) for x in c.ptm[3]][:nph])
    want = []
    for i, p in enumerate(theta):
        a_v = p[c.nspec]
        model = raw[i, 0] * (np.median(spec) / np.median(raw[i, 0]))               # mft6.py:1173
        spec_n = orc.norm_spec(wl, model, spec)                                    # mft6.py:1174
        ic = orc.chisq(model, spec_n, c.err)
        iic = np.sum(ic) / len(ic)
        phot = bands_[i, nc:]
        if a_v > 0 and nph:
            phot = -2.5 * np.log10(orc.extinct(phot_cwl, 10 ** (-0.4 * phot), a_v))  # mft6.py:1163
        chi_c, chi_p = orc.chisq(bands_[i, :nc], c.fr[0], c.fr[1]), orc.chisq(phot, c.fr[3], c.fr[4])
        want.append(-0.5 * np.sum((iic * (nc + nph), np.sum(chi_c), np.sum(chi_p))))   # mft6.py:1191
    close(got, np.array(want), False, 'closure with the hot path, case ' + which)


def test_spectra_of_a_sample_that_cannot_be_evaluated():
    from mcmc_spec_amd import _lib, products
    eng = engine('B')
    theta = goldens()['bin_theta'][:3].copy()
    good = products.spectra(eng, theta)
    theta[1, 0] = 6600.0
    out, scale, status = products.spectra(eng, theta, with_status=True)
    assert list(status) == [0, _lib.W_VALUEERROR, 0] and np.all(np.isnan(out[1])) and np.isnan(scale[1])
    assert np.array_equal(out[[0, 2]], good[0][[0, 2]]) and np.array_equal(scale[[0, 2]], good[1][[0, 2]])
    with pytest.raises(_lib.MsxError):
        products.spectra(engine('B', products=False), theta)


# ---- the drop-in make_composite(plot=True) ---------------------------------------------------------------------------------
def test_make_composite_plot_true_returns_the_references_tuples():
    """Binary (nine entries, mft6.py:816) and triple (eight, :828, magnitudes the six-element arrays of the / zp list)
    against the stored strided window samples and magnitudes; the error when no bands are registered names the call."""
    import mcmc_spec_amd.mft6 as gpu
    from mcmc_spec_amd import bands
    from oracle import mft6_oracle as orc
    g = goldens()
    m = pn.products_matrix()
    idx = g['win_idx']
    gpu.clear_cache()
    gpu.set_product_bands()
    cB, cC = golden_case('B'), golden_case('C')
    gpu.set_band_library(bands.make_bands(cB.tables, *cB.vega))

    def call(c, p, distance=True):
        tt, rad, dist = pn.sample_args(c, p, distance)
        lg = [float(orc.get_logg(t, m)) for t in tt]
        return gpu.make_composite(tt, lg, rad, dist, c.fr[2], c.fr[5], c.r, c.specs, c.ctm, c.ptm, c.tmi, c.tma, None,
                                  nspec=c.nspec, plot=True)
    with pytest.raises(RuntimeError) as e:
        call(cB, g['bin_theta'][0])
    assert 'set_product_bands' in str(e.value) and 'make_composite(plot=True)' in str(e.value)
    gpu.set_product_bands(kepler=(g['kepler_wl'], g['kepler_tm']))
    with pytest.raises(RuntimeError):               # a binary needs the Gaia band too
        call(cB, g['bin_theta'][0])
    gpu.set_product_bands(kepler=(g['kepler_wl'], g['kepler_tm']), gaia=gaia_band(g))
    for i in (0, 2, 4):
        out = call(cB, g['bin_theta'][i])
        assert len(out) == 9
        w, spec1, pri, sec = out[:4]
        assert len(w) == int(g['win_len'][0]) and w[0] == g['win_wl_ends'][0] and w[-1] == g['win_wl_ends'][1]
        assert np.array_equal(spec1, pri + sec)
        close(np.array(out[4:9], dtype=float), g['bin_mags'][i], True, 'plot=True magnitudes, binary sample {}'.format(i))
        if i == 0:
            close(np.array([pri[idx], sec[idx]]), g['win_bin'], False, 'plot=True window, binary')
    out = call(cA := golden_case('A'), g['nod_theta'][1], distance=False)   # distance=False: [ratio], False (mft6.py:2498)
    close(np.array(out[4:9], dtype=float), g['nod_mags'][1], True, 'plot=True magnitudes, distance=False')
    for i in (0, 1):
        out = call(cC, g['tri_theta'][i])
        assert len(out) == 8 and all(np.shape(x) == (6,) for x in out[5:])
        assert np.array_equal(out[1], out[2] + out[3] + out[4])
        close(np.array(out[5:8]), g['tri_mags'][i], True, 'plot=True magnitudes, triple sample {}'.format(i))
        if i == 0:
            close(np.array([a[idx] for a in out[2:5]]), g['win_tri'], False, 'plot=True window, triple')
    # plot=False is what it was
    tt, rad, dist = pn.sample_args(cB, g['bin_theta'][0], True)
    lg = [float(orc.get_logg(t, m)) for t in tt]
    assert len(gpu.make_composite(tt, lg, rad, dist, cB.fr[2], cB.fr[5], cB.r, cB.specs, cB.ctm, cB.ptm, cB.tmi, cB.tma, None)) == 5
    gpu.set_product_bands()
    gpu.clear_cache()
