"""GPU: adaptive temperature ladders on the device-resident sampler (include/msx.h, msx_ladder_adapt / _betas / _current;
csrc/tempered_kernels.h, tempered_adapt_kernel).  The ladder is device state that a one-workgroup
kernel moves after every sweep, so (a) the device must walk the chain AND the ladders of the adaptive host loop fed the
device's own draws, at the shapes where the new kernel and the two adaptive instantiations can go wrong, (b) and of the host
loop with the same seed when the host draws, (c) a frozen ladder is a fixed ladder, (d) the device series hold the same rows
and the evidence is refused over a moving ladder, (e) a loop left early leaves the ladder behind everything queued, and (f)
the ABI refuses what it must."""
import numpy as np
import pytest

import common  # noqa: F401
from test_gpu_tempered import CHUNK, SEED, mix, same_run, start

pytestmark = pytest.mark.gpu

LAG, TIME = 8.0, 2.0
ADAPT = dict(adaptive=True, adaptation_lag=LAG, adaptation_time=TIME)


def device(eng, nw, betas, rng='device', **kw):
    from mcmc_spec_amd.tempered import DeviceTemperedSampler
    return DeviceTemperedSampler(nw, 6, eng, betas=betas, seed=SEED, chunk=CHUNK, rng=rng, moves=mix(), **kw)


def twin_of(eng, nw, betas, seeds, **kw):
    from mcmc_spec_amd.tempered import TemperedSampler
    return TemperedSampler(nw, 6, eng, betas=betas, seeds=seeds, moves=mix(),
                           draws=lambda i, m: eng.ctx.tempered_draw(seeds, mix(), i, m, nw, 6), **kw)


def gathered(p0):
    """The start drawn towards its first walker, walker w by 10^-2 .. 10^-7 (convex combinations: inside the prior).  54
    walkers spread over the whole prior differ in ln L by thousands, and every accept and swap is decided by a sign whatever
    the rung's beta; here the differences span every magnitude, so a rung whose beta moved walks another chain."""
    w0 = p0[0, 0].copy()
    eps = 10.0 ** -np.linspace(2.0, 7.0, p0.shape[1])
    return w0 + eps[None, :, None] * (p0 - w0)


def ladders(s):
    return s.get_betas().copy(), s.betas.copy(), s.ladder_skipped, s._adapted


def two_adaptive_runs(s, p0):
    """test_gpu_tempered.two_runs, with the ladders of the first run kept too."""
    st = s.run_mcmc(p0, 5)
    first = (s.get_chain(t=None).copy(), s.get_log_like(t=None).copy(), s.get_log_prior(t=None).copy(), s.acceptance_fraction.copy(),
             s.swap_fraction.copy(), st)
    lad = ladders(s)
    s.reset()
    s.run_mcmc(st, 6)
    return first, lad


def same_ladders(a, b):
    assert a[0].shape == b[0].shape and a[0].tobytes() == b[0].tobytes()
    assert a[1].tobytes() == b[1].tobytes() and a[2:] == b[2:]


# ---- (a) device-drawn ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,nw', [(3, 18), (2, 18), (8, 258), (64, 12)])
def test_the_adaptive_ladder_walks_the_host_twins_chain_and_ladders(T, nw):
    """(3, 18): one free rung, a fraction of a wave.  (2, 18): nothing is free -- the ladder must not move, the rows are still
    written.  (8, 258): the sweep spans two workgroups, so an iteration's counts come from two blocks' atomics.  (64, 12): one
    thread per rung fills the adapt kernel's workgroup (12 walkers: the fewest the samplers take at ndim 6)."""
    from mcmc_spec_amd.tempered import default_betas
    eng, p0 = start(nw, T)
    if nw == 18:
        p0 = gathered(p0)
    betas = default_betas(T, 0.02)
    dev = device(eng, nw, betas, **ADAPT)
    fd, ld = two_adaptive_runs(dev, p0)
    host = twin_of(eng, nw, betas, dev.seeds, **ADAPT)
    fh, lh = two_adaptive_runs(host, p0)
    same_run(dev, fd, host, fh)
    same_ladders(ld, lh)
    same_ladders(ladders(dev), ladders(host))
    assert dev._adapted == 11 == host._adapted and dev._drawn == 11 and ld[3] == 5
    assert ld[0].shape == (5, T) and dev.get_betas().shape == (6, T)
    assert np.array_equal(ld[0][0], betas) and np.array_equal(dev.get_betas()[0], ld[1])      # each run starts where the last ended
    assert np.all(dev.get_betas()[:, 0] == 1.0) and np.all(dev.get_betas()[:, -1] == betas[-1]) and np.all(np.diff(dev.get_betas(), axis=1) < 0)
    print('T', T, 'nw', nw, 'ladder after 11 iterations', dev.betas, 'skipped', dev.ladder_skipped)
    if T == 2:
        assert np.all(ld[0] == betas) and np.all(dev.get_betas() == betas) and np.array_equal(dev.betas, betas)
        return
    if (T, nw) in ((3, 18), (8, 258)):
        assert not np.array_equal(dev.betas[1:-1], betas[1:-1]) and not np.array_equal(ld[1], betas)      # the ladder moved, in both runs
        fixed = device(eng, nw, betas)
        ff = two_adaptive_runs(fixed, p0)[0]
        assert np.array_equal(ff[0][0], fd[0][0]) and np.array_equal(ff[1][0], fd[1][0])           # the first iteration is the fixed ladder's
        both = [np.concatenate([f[0][1:], s_.get_chain(t=None)]) for f, s_ in ((ff, fixed), (fd, dev))]
        print('iterations whose rows differ from the fixed ladder\'s:', [i + 1 for i in range(10) if not np.array_equal(both[0][i], both[1][i])])
        assert not np.array_equal(both[0], both[1])                                                 # ... and the rest is not
        assert np.all(fixed.get_betas() == betas) and fixed._adapted == 0 and fixed.ladder_skipped == 0


# ---- (b) host-drawn --------------------------------------------------------------------------------------------------------------
def test_the_host_drawn_adaptive_ladder_walks_the_host_loops_chain():
    from mcmc_spec_amd.tempered import TemperedSampler, default_betas
    eng, p0 = start(18, 3)
    betas = default_betas(3, 0.02)
    dev = device(eng, 18, betas, rng='host', **ADAPT)
    fd, ld = two_adaptive_runs(dev, p0)
    host = TemperedSampler(18, 6, eng, betas=betas, seed=SEED, moves=mix(), **ADAPT)
    fh, lh = two_adaptive_runs(host, p0)
    same_run(dev, fd, host, fh)
    same_ladders(ld, lh)
    same_ladders(ladders(dev), ladders(host))
    assert dev._adapted == 11 and not np.array_equal(dev.betas, betas)


# ---- (c) freeze ------------------------------------------------------------------------------------------------------------------
def test_a_frozen_ladder_is_a_fixed_ladder():
    from mcmc_spec_amd.tempered import default_betas
    eng, p0 = start(18, 3)
    betas = default_betas(3, 0.02)
    dev = device(eng, 18, betas, **ADAPT)
    st = dev.run_mcmc(p0, 6)
    adapted = dev.betas.copy()
    assert not np.array_equal(adapted, betas) and dev._adapted == 6
    dev.reset()
    dev.run_mcmc(st, 6, adapt=False)
    assert dev._adapted == 6 and np.array_equal(dev.betas, adapted) and dev.get_betas().shape == (6, 3) and np.all(dev.get_betas() == adapted)
    new = device(eng, 18, adapted)
    new._drawn = 6
    new.run_mcmc(st, 6)
    assert np.array_equal(new.get_chain(t=None), dev.get_chain(t=None)) and np.array_equal(new.get_log_like(t=None), dev.get_log_like(t=None))
    assert np.array_equal(new.get_log_prior(t=None), dev.get_log_prior(t=None))
    assert np.array_equal(new.swap_fraction, dev.swap_fraction) and np.array_equal(new.acceptance_fraction, dev.acceptance_fraction)


# ---- (d) the device series and the evidence ----------------------------------------------------------------------------------------
def test_the_series_hold_an_adaptive_runs_rows_and_the_evidence_wants_a_frozen_ladder():
    from mcmc_spec_amd.tempered import default_betas
    from test_gpu_tempered_series import host_copy, series_hold_the_host_rows
    eng, p0 = start(12, 3)
    dev = device(eng, 12, default_betas(3, 0.02), autocorr='device', **ADAPT)
    st = dev.run_mcmc(p0, 6)
    series_hold_the_host_rows(dev)
    dev.run_mcmc(st, 10, adapt=False)
    series_hold_the_host_rows(dev)
    assert dev.get_betas().shape == (16, 3) and np.all(dev.get_betas()[6:] == dev.betas) and not np.array_equal(dev.get_betas()[1], dev.betas)
    h = host_copy(dev)
    for method in ('ti', 'ss'):
        for kw in (dict(), dict(discard=5), dict(discard=2, thin=4)):
            with pytest.raises(ValueError, match='ladder'):
                dev.log_evidence(method=method, blocks=2, **kw)
        got, want = dev.log_evidence(method=method, discard=6, blocks=2), h.log_evidence(method=method, discard=6, blocks=2)
        scale = max(1.0, abs(want.log_z))
        print(method, got, want)
        assert abs(got.log_z - want.log_z) <= 1e-12 * scale and np.isfinite(got.log_z)
        assert np.all(np.abs(got.mean_log_like - want.mean_log_like) <= 1e-12 * np.maximum(1.0, np.abs(want.mean_log_like)))
        assert abs(got.mc_error - want.mc_error) <= 1e-10 * scale and abs(got.ladder_error - want.ladder_error) <= 1e-10 * scale
    assert np.allclose(dev.mean_log_like(), h.mean_log_like(), rtol=1e-12, atol=0)          # answers over the moving rows too


# ---- (e) a loop left early ---------------------------------------------------------------------------------------------------------
def test_a_loop_left_early_leaves_the_ladder_behind_everything_queued():
    from mcmc_spec_amd.tempered import default_betas
    eng, p0 = start(18, 3)
    betas = default_betas(3, 0.02)
    dev = device(eng, 18, betas, **ADAPT)
    for i, _ in enumerate(dev.sample(p0, iterations=12)):
        if i == 1:                                   # inside the first chunk of 4; the second is queued
            break
    host = twin_of(eng, 18, betas, dev.seeds, **ADAPT)
    st = host.run_mcmc(p0, 8)
    assert dev._adapted == 8 == host._adapted and dev._drawn == 8 and dev.iteration == 2
    assert dev.betas.tobytes() == host.betas.tobytes() and dev.ladder_skipped == host.ladder_skipped
    assert np.array_equal(dev.get_chain(t=None), host.get_chain(t=None)[:2]) and dev.get_betas().tobytes() == host.get_betas()[:2].tobytes()
    dev.reset(), host.reset()
    dev.run_mcmc(st, 5), host.run_mcmc(st, 5)
    assert np.array_equal(dev.get_chain(t=None), host.get_chain(t=None)) and np.array_equal(dev.get_log_like(t=None), host.get_log_like(t=None))
    same_ladders(ladders(dev), ladders(host))
    assert dev._adapted == 13 and np.array_equal(dev.swap_fraction, host.swap_fraction)


# ---- (f) the ABI -------------------------------------------------------------------------------------------------------------------
def test_refusals_and_the_ladder_getters_through_the_abi():
    """msx_ladder_betas on a FIXED run returns the begin ladder in every row (include/msx.h)."""
    from mcmc_spec_amd import _lib
    nw, T = 18, 3
    eng, p0 = start(nw, T)
    ctx = eng.ctx
    flat = p0.reshape(-1, 6)
    lpr, ll = ctx.logprob_batch(flat, _lib.MODE_LOGPRIOR)[0].reshape(T, nw), ctx.logprob_batch(flat, _lib.MODE_LOGLIKE)[0].reshape(T, nw)
    seeds = [SEED, SEED + 1, SEED + 2]
    betas = np.array([1.0, 0.5, 0.25])

    def raises(code, fn, *a):
        with pytest.raises(_lib.MsxError) as ei:
            fn(*a)
        assert ei.value.code == code, ei.value

    twin = _twin_from(eng, seeds, betas, p0, 7)
    ctx.sampler_policy(0)
    try:
        raises(_lib.MSX_ERR_STATE, ctx.tempered_adapt, LAG, TIME, 0)                     # no run
        raises(_lib.MSX_ERR_STATE, ctx.tempered_ladder)
        ctx.tempered_begin(betas, p0, ll, lpr, 2)
        for lag, time, k0 in ((0.0, TIME, 0), (-1.0, TIME, 0), (float('nan'), TIME, 0), (float('inf'), TIME, 0), (LAG, 0.5, 0),
                              (LAG, float('nan'), 0), (LAG, float('inf'), 0), (LAG, TIME, -1)):
            raises(_lib.MSX_ERR_INVALID, ctx.tempered_adapt, lag, time, k0)
        # a fixed run: the begin ladder from both getters, k = skipped = 0
        got, k, skipped = ctx.tempered_ladder()
        assert np.array_equal(got, betas) and (k, skipped) == (0, 0)
        raises(_lib.MSX_ERR_STATE, ctx.tempered_betas, 0, 2)                             # nothing collected yet
        ctx.tempered_enqueue_drawn(0, 2, seeds, mix(), 0)
        raises(_lib.MSX_ERR_STATE, ctx.tempered_adapt, LAG, TIME, 0)                     # after an enqueue
        raises(_lib.MSX_ERR_STATE, ctx.tempered_betas, 0, 2)                             # a chunk is in the slot
        fixed = ctx.tempered_collect(0, 2)
        assert np.array_equal(ctx.tempered_betas(0, 2), np.tile(betas, (2, 1)))
        raises(_lib.MSX_ERR_INVALID, ctx.tempered_betas, 2, 2)
        ctx.tempered_end()
        # an adaptive run: adapt once; the getters follow the run
        ctx.tempered_begin(betas, p0, ll, lpr, 2)
        ctx.tempered_adapt(LAG, TIME, 7)
        raises(_lib.MSX_ERR_STATE, ctx.tempered_adapt, LAG, TIME, 7)                     # twice
        got, k, skipped = ctx.tempered_ladder()
        assert np.array_equal(got, betas) and (k, skipped) == (7, 0)
        ctx.tempered_enqueue_drawn(0, 2, seeds, mix(), 0)
        ctx.tempered_enqueue_drawn(1, 2, seeds, mix(), 2)
        moved = ctx.tempered_collect(0, 2)
        rows = ctx.tempered_betas(0, 2)
        assert np.array_equal(moved[0][0], fixed[0][0]) and np.array_equal(moved[1][0], fixed[1][0])       # the first iteration is the fixed run's
        ctx.tempered_collect(1, 2)
        last = ctx.tempered_betas(1, 2)
        got, k, skipped = ctx.tempered_ladder()
        assert k == 11 and skipped == 0 and np.array_equal(ctx.tempered_betas(0, 2), rows)          # slot 0's rows stay until it is enqueued again
        # the host loop from k = 7 on the device's draws: the four ladders the iterations ran with, and the one behind them
        assert np.vstack([rows, last]).tobytes() == twin.get_betas().tobytes() and got.tobytes() == twin.betas.tobytes()
        assert np.array_equal(rows[0], betas) and np.all(np.vstack([rows, last])[:, [0, 2]] == betas[[0, 2]])
    finally:
        ctx.tempered_end()
        ctx.sampler_policy(-1)


def _twin_from(eng, seeds, betas, p0, k0):
    """The adaptive host loop on the device's draws, 4 iterations from k = k0."""
    from mcmc_spec_amd.tempered import TemperedSampler
    nw = p0.shape[1]
    h = TemperedSampler(nw, 6, eng, betas=betas, seeds=seeds, moves=mix(), draws=lambda i, m: eng.ctx.tempered_draw(seeds, mix(), i, m, nw, 6), **ADAPT)
    h._adapted = k0
    h.run_mcmc(p0, 4)
    return h
