"""GPU: the device-resident pre-optimiser (``optimizer.fit_spec_device`` over ``msx_opt_run_*``) against the
reference's own ``fit_spec`` run (golden case B, ``D_*``), against the host loop ``fit_spec_batch`` chain by chain,
under different chunkings, and in its error convention."""
import os

import numpy as np
import pytest

import common
from common import golden_case, rel_err
import test_opt_device_abi as cpu

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
TLIM = [3000.0, 4200.0]
DIST_PRIOR = (2.0732e-3, 0.0277e-3)


def staged_engine(c, specs=None):
    from mcmc_spec_amd import bands
    from mcmc_spec_amd.engine import Engine
    eng = Engine(0)
    eng.stage_specs(c.specs if specs is None else specs)
    eng.stage_problem(c.data, c.err, c.fr, c.r, c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=c.nspec,
                      bands=bands.make_bands(c.tables, *c.vega))
    return eng


def test_resident_trajectory_matches_the_reference(tmp_path):
    """The assertions tests/test_gpu_parity.py::test_fit_spec_trajectory_matches_the_reference makes of the host loop,
    made of the resident run: the reference's fit_spec with seed 123, its chi^2 file, best point and parameter file."""
    from mcmc_spec_amd import optimizer
    c = golden_case('B')
    g = c.g
    eng = staged_engine(c)
    st = g['D_start']
    res = optimizer.fit_spec_device(eng, st[None, :], TLIM, DIST_PRIOR, c.matrix, common.av_table_exact(), nspec=2,
                                    steps=int(g['D_steps'][0]), dist_fit=True, rad_prior=True,
                                    rngs=[np.random.default_rng(123)], dirname=str(tmp_path))
    line, best_chi, ch = res[0]
    ref = g['D_chisq']
    assert len(ch.savechi) - 1 == len(ref)
    e1 = rel_err(np.array(ch.savechi[1:]), ref[:, 0]).max()
    e2 = rel_err(np.array(ch.savetest[:len(ref) - 3]), ref[3:, 1]).max()
    e3 = rel_err(best_chi, g['D_best_chi'][0])
    e4 = rel_err(np.array([float(x) for x in line.split()]), g['D_best']).max()
    got_params = np.loadtxt(tmp_path / 'params0.txt')
    print('reference: savechi {:.3e} savetest {:.3e} best_chi {:.3e} best {:.3e}'.format(e1, e2, float(e3), e4))
    assert e1 < TIGHT and e2 < TIGHT and e3 < TIGHT
    assert e4 < 1e-12
    assert got_params.shape == g['D_params'].shape and rel_err(got_params, g['D_params']).max() < 1e-12


def real_starts(nspec, nch, seed):
    """cpu.make_starts' start points (the first seven beside the box's edges), every one checked to be in bounds."""
    from mcmc_spec_amd import optimizer
    s = cpu.make_starts(nspec, nch, seed)
    for row in s:
        assert optimizer._in_bounds(optimizer._groups(row, nspec), TLIM)
    return s


def both_runs(c, nspec, steps, nch, seed, rad_prior, dist_fit, tmp_path, chunk=64):
    from mcmc_spec_amd import optimizer
    eng = staged_engine(c)
    starts = real_starts(nspec, nch, seed)
    hd, dd = tmp_path / 'host', tmp_path / 'dev'
    hd.mkdir()
    dd.mkdir()
    rngs = [np.random.default_rng(77 * seed + k) for k in range(nch)]
    rec = cpu.Recorder(rngs)
    host = optimizer.fit_spec_batch(eng, starts, TLIM, DIST_PRIOR, c.matrix, common.av_table_exact(), nspec=nspec, steps=steps,
                                    dist_fit=dist_fit, rad_prior=rad_prior, rngs=rngs, propose=rec, dirname=str(hd))
    rngs = [np.random.default_rng(77 * seed + k) for k in range(nch)]
    dev = optimizer.fit_spec_device(eng, starts, TLIM, DIST_PRIOR, c.matrix, common.av_table_exact(), nspec=nspec, steps=steps,
                                    dist_fit=dist_fit, rad_prior=rad_prior, rngs=rngs, dirname=str(dd), chunk=chunk)
    return host, dev, rec, hd, dd


def assert_same_chains(host, dev, hd, dd, nspec):
    from mcmc_spec_amd import optimizer
    worst = 0.0
    for k, ((hl, hb, hc), (dl, db, dc)) in enumerate(zip(host, dev)):
        assert len(hc.sp) == len(dc.sp), k
        assert all(np.array_equal(cpu.flat(a), cpu.flat(b)) for a, b in zip(hc.sp, dc.sp)), k   # accepted rows: exactly
        hflags = [optimizer.TRIP_ACCEPTED if t < s else optimizer.TRIP_REJECTED for t, s in zip(hc.savetest, hc.savechi)]
        assert hflags == dc.flags, k
        assert hc.n == dc.n and hc.total_n == dc.total_n, k
        assert hl == dl, k
        worst = max(worst, rel_err(np.array(dc.savechi), np.array(hc.savechi)).max(),
                    rel_err(np.array(dc.savetest), np.array(hc.savetest)).max() if hc.savetest else 0.0)
        for name in ('params{}.txt'.format(k),):
            hp, dp = hd / name, dd / name
            assert hp.exists() == dp.exists(), name
            if hp.exists():
                assert hp.read_text() == dp.read_text(), name
    print('host loop vs resident: savechi / savetest worst relative difference {:.3e}'.format(worst))
    assert worst < 1e-12


@pytest.mark.parametrize('rad_prior,dist_fit', [(True, True), (False, False), (True, False), (False, True)])
def test_resident_binaries_walk_the_host_loops_chains(rad_prior, dist_fit, tmp_path):
    c = golden_case('B')
    steps = 12
    host, dev, rec, hd, dd = both_runs(c, 2, steps, 64, 3, rad_prior, dist_fit, tmp_path)
    got = cpu.coverage_of(host, rec, 2, steps)
    print('coverage:', sorted(got))
    assert_same_chains(host, dev, hd, dd, 2)
    want = {'T loop', 'A_V loop', 'radius loop', 'parallax loop', 'coarse accept', 'fine accept', 'ends by n', 'ends by cap'}
    assert want <= got, sorted(want - got)


def test_resident_triples_walk_the_host_loops_chains(tmp_path):
    c = golden_case('C')
    steps = 9  # odd: n = steps / 2 + 1 is fractional
    host, dev, rec, hd, dd = both_runs(c, 3, steps, 64, 3, True, True, tmp_path)
    got = cpu.coverage_of(host, rec, 3, steps)
    print('coverage:', sorted(got))
    assert_same_chains(host, dev, hd, dd, 3)
    assert {'third-radius fix', 'coarse accept', 'ends by n'} <= got, sorted(got)


def test_chunking_changes_nothing_and_the_context_is_left_as_it_was():
    from mcmc_spec_amd import optimizer, _lib
    c = golden_case('B')
    eng = staged_engine(c)
    nch, steps = 8, 12
    starts = real_starts(2, nch, 5)
    th = c.theta[:6]
    before_lp = eng.logposterior(th)
    eng.ctx.opt_init(starts)
    before_os, _ = eng.ctx.opt_step(th, np.arange(6, dtype=np.int32))

    def run(chunk):
        rngs = [np.random.default_rng(900 + k) for k in range(nch)]
        return optimizer.fit_spec_device(eng, starts, TLIM, DIST_PRIOR, c.matrix, common.av_table_exact(), nspec=2, steps=steps,
                                         dist_fit=True, rad_prior=True, rngs=rngs, chunk=chunk)
    runs = {chunk: run(chunk) for chunk in (1, 37, 700)}   # the last: longer than any run (at most 50 * steps draws per chain)
    # (some chain evaluates more proposals than a chunk of 37 trips holds: its run goes on through a chunk's end)
    assert max(len(ch.savetest) for _, _, ch in runs[37]) > 37
    for chunk in (1, 700):
        for (l0, b0, c0), (l1, b1, c1) in zip(runs[37], runs[chunk]):
            assert l0 == l1 and b0 == b1 and c0.n == c1.n and c0.total_n == c1.total_n, chunk
            assert c0.flags == c1.flags and c0.savechi == c1.savechi and c0.savetest == c1.savetest, chunk
            assert all(np.array_equal(cpu.flat(a), cpu.flat(b)) for a, b in zip(c0.sp, c1.sp)), chunk
    # chains that finish early stay idle: straight at the entry points, a second run on the same context
    ctx = eng.ctx
    like0, _ = ctx.opt_init(starts)
    chi0 = np.array([optimizer._initial_chi(like0[k], starts[k], DIST_PRIOR, c.matrix, common.av_table_exact(), 2, True, False)
                     for k in range(nch)])
    ctx.opt_run_begin(starts, chi0, steps, TLIM, True, False, DIST_PRIOR, common.av_table_exact(), None, 700)
    rngs = [np.random.default_rng(900 + k) for k in range(nch)]
    z = np.stack([r.standard_normal((700, 6)) for r in rngs], axis=1)
    ctx.opt_run_enqueue(0, z)
    rec, fl, live, worst = ctx.opt_run_collect(0, 700)
    gi, chi, n, tot = ctx.opt_run_end()
    assert live == 0 and worst <= _lib.W_REJECT
    first_idle = []
    for k in range(nch):
        idle = np.nonzero(fl[:, k] == optimizer.TRIP_IDLE)[0]
        assert idle.size > 0 and np.all(fl[idle[0]:, k] == optimizer.TRIP_IDLE), k
        assert np.all(rec[idle[0]:, k, :7] == rec[idle[0] - 1, k, :7]) and np.all(np.isnan(rec[idle[0]:, k, 7])), k
        assert np.array_equal(rec[-1, k, :6], gi[k]) and rec[-1, k, 6] == chi[k]
        assert n[k] >= steps or tot[k] >= 50 * steps
        first_idle.append(int(idle[0]))
    assert len(set(first_idle)) > 1  # they did not all finish in the same trip
    # existing launches after the runs: the bits they returned before them
    assert np.array_equal(eng.logposterior(th), before_lp)
    eng.ctx.opt_init(starts)
    after_os, _ = eng.ctx.opt_step(th, np.arange(6, dtype=np.int32))
    assert np.array_equal(after_os, before_os)


def test_entry_points_check_their_arguments_before_any_device_work():
    from mcmc_spec_amd import optimizer, _lib
    c = golden_case('B')
    eng = staged_engine(c)
    ctx = eng.ctx
    starts = real_starts(2, 4, 5)
    av = common.av_table_exact()
    with pytest.raises(_lib.MsxError):   # no msx_opt_init yet
        ctx.opt_run_begin(starts, np.zeros(4), 12, TLIM, True, False, DIST_PRIOR, av, None, 8)
    ctx.opt_init(starts)
    with pytest.raises((_lib.MsxError, ValueError)):      # one chain per row of msx_opt_init's theta0
        ctx.opt_run_begin(starts[:3], np.zeros(3), 12, TLIM, True, False, DIST_PRIOR, av, None, 8)
    with pytest.raises((_lib.MsxError, ValueError)):      # rad_prior without the isochrone
        ctx.opt_run_begin(starts, np.zeros(4), 12, TLIM, True, True, DIST_PRIOR, av, None, 8)
    ctx.opt_run_begin(starts, np.full(4, 1e9), 12, TLIM, True, False, DIST_PRIOR, av, None, 8)
    with pytest.raises((_lib.MsxError, ValueError)):      # longer than max_chunk_trips
        ctx.opt_run_enqueue(0, np.zeros((9, 4, 6)))
    with pytest.raises((_lib.MsxError, ValueError)):      # nothing queued in this slot
        ctx.opt_run_collect(1, 8)
    ctx.opt_run_enqueue(0, np.zeros((8, 4, 6)))
    with pytest.raises((_lib.MsxError, ValueError)):      # the slot holds a chunk that was not collected
        ctx.opt_run_enqueue(0, np.zeros((8, 4, 6)))
    rec, fl, live, worst = ctx.opt_run_collect(0, 8)
    # z = 0: every proposal is the start point itself -- better than the chi^2 of 1e9 given for it once, then never again
    assert np.all(fl[0] == optimizer.TRIP_ACCEPTED) and np.all(fl[1:] == optimizer.TRIP_REJECTED)
    assert np.array_equal(rec[0, :, :6], starts) and np.all(rec[1:, :, 6] == rec[0, :, 6]) and live == 4 and worst <= 1
    ctx.opt_init(starts)                # ends the run
    with pytest.raises((_lib.MsxError, ValueError)):
        ctx.opt_run_enqueue(0, np.zeros((8, 4, 6)))


def test_unstaged_node_raises_keyerror_like_the_host_loop():
    """Sparse ``specs`` (as in test_error_conventions): two logg nodes of one Teff are missing; a chain started two
    cells away walks into them.  The resident run raises the host loop's KeyError, naming the same proposal."""
    from mcmc_spec_amd import optimizer
    c = golden_case('B')
    specs = dict(c.specs)
    del specs['3800, 4.5'], specs['3800, 5.0']   # (3800 K stays a node: its other logg entries are there)
    eng = staged_engine(c, specs)
    start = np.array([[3560.0, 3340.0, 0.1, 0.45, 0.6, 2.07e-3]])
    args = (eng, start, TLIM, DIST_PRIOR, c.matrix, common.av_table_exact())
    kw = dict(nspec=2, steps=400, dist_fit=True, rad_prior=False)
    with pytest.raises(KeyError) as host:
        optimizer.fit_spec_batch(*args, rngs=[np.random.default_rng(11)], **kw)
    with pytest.raises(KeyError) as dev:
        optimizer.fit_spec_device(*args, rngs=[np.random.default_rng(11)], **kw)
    assert str(host.value) == str(dev.value)
    # and the context takes the next run
    ok = optimizer.fit_spec_device(staged_engine(c), start, TLIM, DIST_PRIOR, c.matrix, common.av_table_exact(),
                                   rngs=[np.random.default_rng(11)], nspec=2, steps=6, dist_fit=True, rad_prior=False)
    assert ok[0][2].n >= 6 or ok[0][2].total_n >= 300
