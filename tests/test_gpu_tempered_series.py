"""GPU: a tempered run's device series and the evidence reduction (include/msx.h, msx_series_attach_tempered,
msx_series_evidence; csrc/evidence_kernels.h).  (a) An attached run leaves in its two series exactly
the rows msx_tempered_collect returns, host-drawn or device-drawn, over ragged chunks, growth and consecutive runs, and
walks the chain it walks unattached; (b) the other sections' consumers work on those series with rungs as members; (c) the
evidence kernels against their NumPy twin (tests/evidence_numpy.py: the means bit for bit) and an independent reference at
every size where their tiling changes; (d) the ladder's log_evidence against the host's; (e) the ABI refuses what it must
and a refused call leaves the run and the series as they were."""
import numpy as np
import pytest

import common
import evidence_numpy as en
from test_gpu_tempered import BETAS3, SEED, start

pytestmark = pytest.mark.gpu

T = 3
COUNTS = [5, 8, 64]          # the evidence cases' members: less than a wave, an odd size, a wave
DB = np.array([0.0, 0.3, 0.05])


def mix():
    from mcmc_spec_amd.moves import DEMove, StretchMove
    return [(StretchMove(), .5), (DEMove(), .5)]


def ladder(eng, nw, rng, autocorr, chunk=5, cap_hint=0):
    from mcmc_spec_amd.tempered import DeviceTemperedSampler
    return DeviceTemperedSampler(nw, 6, eng, betas=BETAS3, seed=SEED, chunk=chunk, rng=rng, moves=mix(), autocorr=autocorr, cap_hint=cap_hint)


def rows_of(s):
    """(chain (n, T nw, ndim), dens (n, T nw, 2)) of the sampler's HOST copies, in the series' layout."""
    n = len(s._chain)
    return (s.get_chain(t=None).reshape(n, -1, s.ndim),
            np.stack([s.get_log_like(t=None).reshape(n, -1), s.get_log_prior(t=None).reshape(n, -1)], axis=2))


def series_hold_the_host_rows(s):
    chain, dens = rows_of(s)
    assert s._series.rows >= len(chain) and s._dens.rows == s._series.rows
    assert np.array_equal(s._series.read(0, len(chain)), chain) and np.array_equal(s._dens.read(0, len(chain)), dens)


def host_copy(dev):
    """A host ladder holding dev's stored rows: TemperedSampler's own paths (NumPy; uploads for the summaries)."""
    from mcmc_spec_amd.tempered import TemperedSampler
    h = TemperedSampler(dev.nwalkers, dev.ndim, dev.engine, betas=dev.betas, seeds=dev.seeds)
    h._chain, h._ll, h._lpr = list(dev._chain), list(dev._ll), list(dev._lpr)
    return h


NW = 12   # the fewest walkers the samplers take at ndim 6 (the stretch move's nwalkers >= 2 ndim)


def long_run():
    """nw = 12, 310 iterations device-drawn in two runs at cap_hint = 0: the series cross their 256-row growth in flight."""
    if 'tempered_series_long' not in common._cache:
        eng, p0 = start(NW, T)
        s = ladder(eng, NW, 'device', 'device', chunk=64)
        st = s.run_mcmc(p0, 300)
        first = s._series.rows
        s.run_mcmc(st, 10)
        common._cache['tempered_series_long'] = (s, first)
    return common._cache['tempered_series_long']


# ---- (a) the attached run ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('fed', ['host', 'device'])
@pytest.mark.parametrize('nw', [8, 6])
def test_an_attached_run_keeps_the_rows_it_returns(nw, fed):
    """T = 3, nw = 8 and 6, ndim = 6, 23 iterations in chunks of 5 (a ragged last chunk), chunks fed from the host and
    drawn on the device, through the ABI: the samplers refuse fewer than 2 ndim = 12 walkers (the next test is theirs).  The
    series hold what msx_tempered_collect returned, and an unattached run returns the same."""
    from mcmc_spec_amd import _lib
    eng, p0 = start(nw, T)
    ctx = eng.ctx
    flat = p0.reshape(-1, 6)
    lpr, ll = ctx.logprob_batch(flat, _lib.MODE_LOGPRIOR)[0].reshape(T, nw), ctx.logprob_batch(flat, _lib.MODE_LOGLIKE)[0].reshape(T, nw)
    seeds = [SEED, SEED + 1, SEED + 2]
    sizes = [5, 5, 5, 5, 3]

    def run(chain, dens):
        out = []
        ctx.sampler_policy(0)
        ctx.tempered_begin(np.array(BETAS3), p0, ll, lpr, 5)
        try:
            if chain is not None:
                ctx.tempered_attach_series(chain, dens, 0)
            done = 0
            for i, m in enumerate(sizes + [0]):        # two chunks in flight, as the samplers keep them
                if m:
                    if fed == 'device':
                        ctx.tempered_enqueue_drawn(i & 1, m, seeds, mix(), done)
                    else:
                        members, swap_logu = ctx.tempered_draw(seeds, mix(), done, m, nw, 6)
                        ctx.tempered_enqueue(i & 1, *[np.stack([mb[j] for mb in members], axis=1) for j in range(8)], swap_logu)
                    done += m
                if i:
                    out.append(ctx.tempered_collect((i - 1) & 1, sizes[i - 1]))
                    if chain is not None:              # a collected chunk's rows are in place while the next one runs
                        upto = sum(sizes[:i])
                        assert np.array_equal(chain.read(upto - sizes[i - 1], sizes[i - 1]), out[-1][0].reshape(sizes[i - 1], T * nw, 6))
        finally:
            ctx.tempered_end()
            ctx.sampler_policy(-1)
        return [np.concatenate([o[j] for o in out]) for j in range(3)] + [out[-1][3], out[-1][4]]

    chain, dens = _lib.Series(ctx, T * nw, 6, [nw] * T), _lib.Series(ctx, T * nw, 2, [nw] * T)
    got = run(chain, dens)
    assert chain.rows == 23 == dens.rows
    assert np.array_equal(chain.read(), got[0].reshape(23, T * nw, 6))
    assert np.array_equal(dens.read(), np.stack([got[1].reshape(23, -1), got[2].reshape(23, -1)], axis=2))
    plain = run(None, None)
    assert all(np.array_equal(a, b) for a, b in zip(got, plain))
    assert got[3].sum() > 0 and len(np.unique(got[0][:, :, :, 0])) > 23          # (the walkers moved)
    chain.close()
    dens.close()


@pytest.mark.parametrize('rng', ['host', 'device'])
def test_the_samplers_chain_is_the_same_attached_or_not(rng, nw=NW):
    """autocorr='device' against autocorr='host': 23 iterations in chunks of 5."""
    eng, p0 = start(nw, T)
    dev = ladder(eng, nw, rng, 'device')
    dev.run_mcmc(p0, 23)
    assert dev._series.rows == 23 and dev._series.k == T and dev._dens.ndim == 2
    series_hold_the_host_rows(dev)
    plain = ladder(eng, nw, rng, 'host')
    plain.run_mcmc(p0, 23)
    assert plain._series is None
    assert np.array_equal(dev.get_chain(t=None), plain.get_chain(t=None)) and np.array_equal(dev.get_log_like(t=None), plain.get_log_like(t=None))
    assert np.array_equal(dev.get_log_prior(t=None), plain.get_log_prior(t=None)) and np.array_equal(dev.swap_fraction, plain.swap_fraction)
    assert np.array_equal(dev.acceptance_fraction, plain.acceptance_fraction)
    assert len(np.unique(dev.get_chain(t=None)[:, :, :, 0])) > 23          # (the walkers moved)


def test_growth_and_reuse():
    s, first = long_run()
    assert first == 300 and s._series.rows == 310 == len(s._chain)          # the second run appended from len(chain)
    series_hold_the_host_rows(s)
    from mcmc_spec_amd import _lib
    eng, p0 = start(NW, T)
    r = ladder(eng, NW, 'device', 'device', chunk=4)
    st = r.run_mcmc(p0, 9)
    r.reset()
    assert r.get_autocorr_time(quiet=True).shape == (6,) and np.all(np.isnan(r.get_autocorr_time(quiet=True)))
    r.run_mcmc(st, 7)
    assert r._series.rows == 7 == r._dens.rows                             # reset, then sample: from row 0
    series_hold_the_host_rows(r)
    r.run_mcmc(r.get_last_sample(), 2, store=False)                         # not stored: not attached
    assert r._series.rows == 7
    extra = np.full((1, T * NW, 6), 2.5)
    r._series.append(extra)                                                 # detached at the run's end: append works again
    assert r._series.rows == 8 and np.array_equal(r._series.read(7, 1), extra)
    assert isinstance(r._series, _lib.Series)


# ---- (b) the consumers --------------------------------------------------------------------------------------------------------
def test_autocorrelation_and_summary_of_a_rung():
    s, _ = long_run()
    h = host_copy(s)
    for t in (0, T - 1):
        got, want = s.get_autocorr_time(t=t, quiet=True), h.get_autocorr_time(t=t, quiet=True)
        assert got.shape == (6,) and np.all(np.isfinite(want))
        assert np.all(np.abs(got - want) <= 1e-9 * np.abs(want)), (t, got, want)
    every = s.get_autocorr_time(t=None, quiet=True, discard=10, thin=2)
    assert every.shape == (T, 6)
    assert np.all(np.abs(every - h.get_autocorr_time(t=None, quiet=True, discard=10, thin=2)) <= 1e-9 * np.abs(every))
    q = (0.16, 0.5, 0.84)
    for t in (0, T - 1):
        flat = s.get_chain(t=t, flat=True, discard=7, thin=3)
        got = s.get_summary(t=t, q=q, discard=7, thin=3)
        assert np.array_equal(got['quantiles'], np.quantile(flat, q, axis=0).T) and got['count'] == len(flat)
        assert np.array_equal(got['median'], np.median(flat, axis=0)) and np.array_equal(got['min'], flat.min(axis=0))
        up = h.get_summary(t=t, q=q, discard=7, thin=3)                     # the host ladder: uploaded first
        assert all(np.array_equal(got[name], up[name]) for name in got)
    every = s.get_summary(t=None, q=q)
    assert every['quantiles'].shape == (T, 6, 3)
    assert np.array_equal(every['quantiles'][1], np.quantile(s.get_chain(t=1, flat=True), q, axis=0).T)


def test_products_of_a_rung():
    """Two rungs of 16 walkers on the products fixture's engine: the one engine serves every member."""
    from mcmc_spec_amd import products, synth
    from mcmc_spec_amd.tempered import DeviceTemperedSampler
    from test_gpu_products import PRODUCT_COLS, _host_summary, _same, engine
    eng = engine('B')
    c = common.golden_case('B')
    p0 = synth.draw_walkers(32, seed=9, tmin=c.tmin, tmax=c.tmax).reshape(2, 16, 6)
    s = DeviceTemperedSampler(16, 6, eng, betas=[1.0, 0.4], seed=5, chunk=7, rng='device', autocorr='device')
    s.run_mcmc(p0, 20)
    for t in (0, 1):
        vals = products.evaluate(eng, s.get_chain(t=t, discard=2, thin=3, flat=True), PRODUCT_COLS)
        assert np.all(np.isfinite(vals))
        _same(s.get_products(PRODUCT_COLS, t=t, discard=2, thin=3), _host_summary(vals))
    idx = np.random.default_rng(3).choice(len(vals), 50, replace=False)
    _same(s.get_products(PRODUCT_COLS, t=1, discard=2, thin=3, indices=idx), _host_summary(vals[idx]))
    _same(host_copy(s).get_products(PRODUCT_COLS, t=1, discard=2, thin=3), _host_summary(vals))
    assert s.get_products(PRODUCT_COLS, t=None)['quantiles'].shape == (2, 3, 3)


# ---- (c) the evidence kernels ------------------------------------------------------------------------------------------------
NROWS = 3600   # the longest selection: n' = 513 at thin = 7


def appended():
    """Arbitrary rows put in with msx_series_append: (series, rows (NROWS, 77, 2))."""
    if 'evidence_series' not in common._cache:
        from mcmc_spec_amd import _lib
        from test_gpu_overlap import _config2
        eng, _ = _config2()
        rng = np.random.default_rng(21)
        rows = np.stack([rng.normal(-300.0, 40.0, (NROWS, sum(COUNTS))), rng.normal(5.0, 1.0, (NROWS, sum(COUNTS)))], axis=2)
        s = _lib.Series(eng.ctx, sum(COUNTS), 2, COUNTS)
        s.append(rows)
        common._cache['evidence_series'] = (s, rows)
    return common._cache['evidence_series']


def check(series, rows, n, discard, thin, col, db, B):
    x = rows[:n][discard::thin, :, col]
    mean, lme = series.evidence(n, discard, thin, col, db, B)
    tw_mean, tw_lme = en.twin(x, series.counts, db, B)
    ref_mean, ref_lme = en.reference(x, series.counts, db, B)
    assert mean.shape == (series.k, B + 1)
    assert np.array_equal(mean, tw_mean, equal_nan=True), (n, discard, thin, B)
    assert en.close(mean, ref_mean, 1e-9)
    if db is None:
        assert lme is None
    else:
        assert en.close(lme, tw_lme, 1e-12) and en.close(lme, ref_lme, 1e-9), (n, discard, thin, B)
    return mean, lme


# 256 is the kernels' tile (kEvdThreads: a workgroup's stride through its block and the width of its tree): one short of,
# at and one past one and two tiles; B = 1 puts them in ONE block
@pytest.mark.parametrize('np_', [1, 2, 255, 256, 257, 511, 512, 513])
def test_block_means_and_lme_against_the_twin_and_the_reference(np_):
    series, rows = appended()
    for discard, thin in ((0, 1), (3, 2), (0, 7)):
        n = discard + (np_ - 1) * thin + 1
        for B in sorted({1, min(3, np_), np_ if np_ <= 64 else 1}):
            check(series, rows, n, discard, thin, 0, DB, B)
    check(series, rows, np_, 0, 1, 1, None, 1)                 # db = NULL, the other column
    if np_ >= 256:
        check(series, rows, np_, 0, 1, 0, DB, 64)              # every block short of a tile


def test_special_values():
    from mcmc_spec_amd import _lib
    series, rows = appended()
    x = rows[:300].copy()
    x[150, 1, 0] = -np.inf                   # member 0: one -inf, in block 1 of 3
    x[:, 5:13, 0] = -np.inf                  # member 1: all -inf
    x[7, 70, 0] = np.nan                     # member 2: a NaN in block 0
    s = _lib.Series(series_ctx(), sum(COUNTS), 2, COUNTS)
    s.append(x)
    mean, lme = check(s, x, 300, 0, 1, 0, np.array([0.2, 0.3, 0.05]), 3)
    assert mean[0, 0] == -np.inf and mean[0, 2] == -np.inf and np.isfinite(mean[0, 1]) and np.isfinite(mean[0, 3])
    assert np.all(np.isfinite(lme[0]))                                       # a -inf weighs zero
    assert np.all(mean[1] == -np.inf) and np.all(lme[1] == -np.inf)          # never NaN
    assert np.isnan(mean[2, 0]) and np.isnan(mean[2, 1]) and np.isnan(lme[2, 0]) and np.isnan(lme[2, 1])
    assert np.all(np.isfinite(mean[2, 2:])) and np.all(np.isfinite(lme[2, 2:]))
    s.close()


def series_ctx():
    from test_gpu_overlap import _config2
    return _config2()[0].ctx


def test_the_bits_do_not_depend_on_how_the_rows_arrived():
    from mcmc_spec_amd import _lib
    eng, p0 = start(NW, T)
    dev = ladder(eng, NW, 'device', 'device')
    dev.run_mcmc(p0, 23)
    db = np.array([0.0, 0.5, 0.25])
    want = dev._dens.evidence(23, 2, 2, 0, db, 4)
    dens = dev._dens.read(0, 23)
    for cap in (0, 23, 1000):
        s = _lib.Series(eng.ctx, T * NW, 2, [NW] * T, cap_hint=cap)
        s.append(dens[:9])
        s.append(dens[9:])
        got = s.evidence(23, 2, 2, 0, db, 4)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), cap
        s.close()
    assert np.array_equal(want[0], en.twin(dens[2:23:2, :, 0], [NW] * T, db, 4)[0])


# ---- (d) the ladder's evidence --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('method', ['ti', 'ss'])
def test_log_evidence_is_the_host_ladders(method):
    s, _ = long_run()
    h = host_copy(s)
    for kw in (dict(), dict(discard=10, thin=3, blocks=5)):
        got, want = s.log_evidence(method=method, **kw), h.log_evidence(method=method, **kw)
        scale = max(1.0, abs(want.log_z))
        print(method, kw, got, want)
        assert abs(got.log_z - want.log_z) <= 1e-12 * scale
        assert np.all(np.abs(got.mean_log_like - want.mean_log_like) <= 1e-12 * np.maximum(1.0, np.abs(want.mean_log_like)))
        # the two error figures are differences of estimates each good to 1e-12 scale
        assert abs(got.mc_error - want.mc_error) <= 1e-10 * scale and abs(got.ladder_error - want.ladder_error) <= 1e-10 * scale
        assert np.isfinite(got.log_z) and got.mc_error > 0.0
    assert np.allclose(s.mean_log_like(discard=4), h.mean_log_like(discard=4), rtol=1e-12, atol=0)


# ---- (e) refusals -------------------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_series_and_the_run_as_they_were():
    from mcmc_spec_amd import _lib
    series, rows = appended()
    lib, out, out2 = series.lib, np.empty((3, 65)), np.empty((3, 65))

    def evidence(n, discard, thin, col, B):
        return lib.msx_series_evidence(series.h, n, discard, thin, col, _lib.dptr(DB), B, _lib.dptr(out), _lib.dptr(out2))

    before = series.evidence(100, 0, 1, 0, DB, 4)
    for args in ((NROWS + 1, 0, 1, 0, 1), (0, 0, 1, 0, 1), (10, 10, 1, 0, 1), (10, 0, 1, 2, 1), (10, 0, 1, -1, 1), (10, 0, 1, 0, 0),
                 (10, 0, 1, 0, 11), (10, 0, 3, 0, 5), (100, 0, 1, 0, 65)):
        assert evidence(*args) == _lib.MSX_ERR_RANGE, args
    assert evidence(10, -1, 1, 0, 1) == _lib.MSX_ERR_INVALID and evidence(10, 0, 0, 0, 1) == _lib.MSX_ERR_INVALID
    with pytest.raises(ValueError):
        series.evidence(10, 0, 1, 0, DB, 11)
    after = series.evidence(100, 0, 1, 0, DB, 4)
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])

    nw = 8
    eng, p0 = start(nw, T)
    ctx = eng.ctx
    flat = p0.reshape(-1, 6)
    lpr, ll = ctx.logprob_batch(flat, _lib.MODE_LOGPRIOR)[0].reshape(T, nw), ctx.logprob_batch(flat, _lib.MODE_LOGLIKE)[0].reshape(T, nw)
    seeds = [SEED, SEED + 1, SEED + 2]

    def raises(code, fn, *a):
        with pytest.raises(_lib.MsxError) as ei:
            fn(*a)
        assert ei.value.code == code, ei.value

    chain, dens = _lib.Series(ctx, T * nw, 6, [nw] * T), _lib.Series(ctx, T * nw, 2, [nw] * T)
    raises(_lib.MSX_ERR_STATE, ctx.tempered_attach_series, chain, dens, 0)           # no tempered run
    ctx.sampler_policy(0)
    try:
        ctx.tempered_begin(np.array(BETAS3), p0, ll, lpr, 4)
        raises(_lib.MSX_ERR_INVALID, ctx.tempered_attach_series, None, None, 0)
        raises(_lib.MSX_ERR_INVALID, ctx.tempered_attach_series, chain, dens, 1)     # at_row past the rows held
        raises(_lib.MSX_ERR_INVALID, ctx.tempered_attach_series, chain, chain, 0)    # dens needs ndim = 2 (and a series of its own)
        for bad in (_lib.Series(ctx, T * nw, 6), _lib.Series(ctx, T * nw, 6, [nw + 2, nw - 2, nw]), _lib.Series(ctx, 2 * nw, 6, [nw] * 2),
                    _lib.Series(ctx, T * nw, 5, [nw] * T)):
            raises(_lib.MSX_ERR_INVALID, ctx.tempered_attach_series, bad, None, 0)   # k, counts, nw, ndim
            bad.close()
        raises(_lib.MSX_ERR_STATE, ctx.sampler_attach_series, chain, 0)              # (as before: not this run's call)
        assert chain.rows == 0 and dens.rows == 0
        # a refused attach is followed by a normal run: this one goes unattached
        ctx.tempered_enqueue_drawn(0, 4, seeds, mix(), 0)
        raises(_lib.MSX_ERR_STATE, ctx.tempered_attach_series, chain, dens, 0)       # after the first enqueue
        unattached = ctx.tempered_collect(0, 4)
    finally:
        ctx.tempered_end()
    assert chain.rows == 0
    try:
        ctx.tempered_begin(np.array(BETAS3), p0, ll, lpr, 4)
        ctx.tempered_attach_series(chain, None, 0)                                   # the chain alone
        raises(_lib.MSX_ERR_STATE, ctx.tempered_attach_series, None, dens, 0)        # attach once
        raises(_lib.MSX_ERR_STATE, chain.append, np.zeros((1, T * nw, 6)))           # a run in flight appends to it
        ctx.tempered_enqueue_drawn(0, 4, seeds, mix(), 0)
        attached = ctx.tempered_collect(0, 4)
    finally:
        ctx.tempered_end()
        ctx.sampler_policy(-1)
    assert all(np.array_equal(a, b) for a, b in zip(attached, unattached))
    assert chain.rows == 4 and dens.rows == 0 and np.array_equal(chain.read(), attached[0].reshape(4, T * nw, 6))
    chain.close()
    dens.close()
