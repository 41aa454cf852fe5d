"""GPU: the single-target device-drawn sampler beyond its first run (msx_sampler_enqueue_drawn's first_iter;
mcmc_spec_amd.sampler.DeviceEnsembleSampler(rng='device')).  The reference's driver burns in, calls reset() and runs
production, so the generator's stream has to go on across sample() / run_mcmc() calls and reset(): every chain here must be,
bit for bit, the chain the HOST loop walks over the same calls when it is fed the device generator's own numbers
(EnsembleSampler(draws=lambda i, m: ctx.sampler_draw(seed, a, i, m, nw, ndim)), which counts its iterations across calls).

Ensembles: 18 walkers (9 active: a fraction of a wave, the generator's sort pads to 32) and 256 (two half-steps of 128 fill
the chip: the run overlaps its half-steps, and a second run then carries hand-over versions that start at 0 again while the
stream does not).  chunk = 4: runs of 5 and 6 iterations cross a chunk boundary and end on a short chunk."""
import os

import numpy as np
import pytest

import common
from test_gpu_overlap import _config2

pytestmark = pytest.mark.gpu

A, SEED, CHUNK, NDIM = 2.0, 2024, 4, 6
ENSEMBLES = (18, 256)


def p0_of(nw):
    from mcmc_spec_amd import synth
    _, W = _config2()
    return synth.draw_walkers(nw, seed=9 + nw, tmin=W['tmin'], tmax=W['tmax'])


def twin(nw, key=SEED):
    """The host twin: the host loop over the same posterior, fed the device generator's stream of `key`."""
    from mcmc_spec_amd.sampler import EnsembleSampler
    eng, _ = _config2()
    return EnsembleSampler(nw, NDIM, eng.logposterior, vectorize=True, draws=lambda i, m: eng.ctx.sampler_draw(key, A, i, m, nw, NDIM))


def device(nw, seed=SEED, **kw):
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    eng, _ = _config2()
    return DeviceEnsembleSampler(nw, NDIM, eng, seed=seed, chunk=CHUNK, rng='device', **kw)


class Snap:
    """What a comparison reads of a sampler, taken when the run is done (the reference is computed once and not touched)."""

    def __init__(self, s, state):
        self.chain, self.logp = s.get_chain().copy(), s.get_log_prob().copy()
        self.acc = s.acceptance_fraction.copy()
        self.coords, self.log_prob = state.coords.copy(), state.log_prob.copy()
        for x in (self.chain, self.logp, self.acc, self.coords, self.log_prob):
            x.flags.writeable = False


def same(dev, state, ref):
    assert dev.get_chain().shape == ref.chain.shape
    assert np.array_equal(dev.get_chain(), ref.chain)
    assert np.array_equal(dev.get_log_prob(), ref.logp)
    assert np.array_equal(state.coords, ref.coords) and np.array_equal(state.log_prob, ref.log_prob)
    assert np.array_equal(dev.acceptance_fraction, ref.acc)


def reference(nw, reset):
    """The twin's run of 5 iterations, (reset(),) and 6 more: (Snap after the first run, Snap after the second)."""
    key = ('sampler_runs', nw, reset)
    if key not in common._cache:
        es = twin(nw)
        st = es.run_mcmc(p0_of(nw), 5)
        first = Snap(es, st)
        if reset:
            es.reset()
        second = Snap(es, es.run_mcmc(st, 6))
        assert es._drawn == 11 and 0.05 < second.acc.mean() < 0.95
        common._cache[key] = (first, second)
    return common._cache[key]


# ---- 1. continuation ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('overlap', [None, False], ids=['default', 'plain'])
@pytest.mark.parametrize('nw', ENSEMBLES)
def test_a_second_run_continues_the_stream(nw, overlap):
    first, second = reference(nw, False)
    dev = device(nw, overlap=overlap)
    st = dev.run_mcmc(p0_of(nw), 5)
    same(dev, st, first)
    assert dev._drawn == 5
    st = dev.run_mcmc(st, 6)
    # (256 walkers under the default policy: the versions of an overlapped run at a stream position that is not 0)
    assert dev.overlapped is (overlap is None)
    assert dev._drawn == 11 and dev.get_chain().shape == (11, nw, NDIM)
    same(dev, st, second)


# ---- 2. reset() does not rewind ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('nw', ENSEMBLES)
def test_reset_does_not_rewind_the_stream(nw):
    first, second = reference(nw, True)
    dev = device(nw)
    st = dev.run_mcmc(p0_of(nw), 5)
    dev.reset()
    assert dev._drawn == 5 and dev.iteration == 0
    st2 = dev.run_mcmc(st, 6)
    assert dev.get_chain().shape == (6, nw, NDIM)
    same(dev, st2, second)
    fresh = device(nw)                   # (the same seed from iteration 0: what the second run must NOT walk)
    fresh.run_mcmc(st, 6)
    assert fresh.get_chain().shape == (6, nw, NDIM) and not np.array_equal(fresh.get_chain(), dev.get_chain())


# ---- 3. one iteration at a time -------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nw', ENSEMBLES)
def test_six_runs_of_one_iteration_are_one_run_of_six(nw):
    first, second = reference(nw, False)
    whole = device(nw)
    ws = whole.run_mcmc(p0_of(nw), 6)
    step = device(nw)
    st, states = p0_of(nw), []
    for i in range(6):
        st = step.run_mcmc(st, 1)
        states.append(st.coords.copy())
        assert step._drawn == i + 1
    assert np.array_equal(step.get_chain(), whole.get_chain()) and np.array_equal(step.get_log_prob(), whole.get_log_prob())
    assert np.array_equal(st.coords, ws.coords) and np.array_equal(st.log_prob, ws.log_prob)
    assert np.array_equal(step.acceptance_fraction, whole.acceptance_fraction)
    assert np.array_equal(whole.get_chain(), second.chain[:6]) and np.array_equal(whole.get_log_prob(), second.logp[:6])
    # six different moves, six different states
    for i in range(6):
        for j in range(i):
            assert not np.array_equal(states[i], states[j]), (i, j)


# ---- 4. the reference's protocol ---------------------------------------------------------------------------------------------
def _files(d):
    return {name: open(os.path.join(d, name), 'rb').read() for name in sorted(os.listdir(d))}


PROTOCOL_SCALE = 0.03


def tight_p0(nw):
    """PROTOCOL_SCALE of draw_walkers' spread about its centre: an ensemble whose twin has no walker sitting still through
    the rows of an autocorrelation check (protocol_reference asserts it)."""
    from mcmc_spec_amd import synth
    return synth.TRUTH_THETA + PROTOCOL_SCALE * (p0_of(nw) - synth.TRUTH_THETA)


def protocol_reference(nw, tmp_path_factory):
    """The twin's protocol run: (samples, files, production chain).  Device and host autocorrelation agree to roundoff only
    on series that move: a constant series has autocorrelation 1 at every lag on the device and the rounding residue's in
    the host's FFT (two definitions, whoever draws).  So the ensemble is one in which every walker
    has moved within the rows of every check, which is asserted here, on the twin's chain."""
    from mcmc_spec_amd.sampler import run_reference_protocol
    key = ('sampler_runs_protocol', nw)
    if key not in common._cache:
        d = str(tmp_path_factory.mktemp('twin{}'.format(nw)))
        es = twin(nw)
        samples = run_reference_protocol(es, tight_p0(nw), nburn=7, nsteps=40, nthin=10, dirname=d)
        chain = es.get_chain().copy()
        assert chain.shape == (40, nw, NDIM)
        for n in (10, 20, 30):
            rows = chain[:n + 1]
            assert not np.any(np.all(rows == rows[0], axis=(0, 2))), 'a walker sits still through the check at n = {}'.format(n)
        common._cache[key] = (samples, _files(d), chain)
    return common._cache[key]


@pytest.mark.parametrize('autocorr', ['host', 'device'])
@pytest.mark.parametrize('nw', ENSEMBLES)
def test_the_reference_protocol_end_to_end(nw, autocorr, tmp_path, tmp_path_factory):
    """Burn-in (7: a whole chunk and a short one), reset(), production (40) with the autocorrelation time every 10
    iterations.  autocorr='host': every file identical.  autocorr='device': samples and coordinate dumps identical, the
    autocorr lines (str(mean tau), one per check) to 1e-9 relative -- the device's direct sums against the host's FFT,
    the tolerance of tests/test_gpu_group_rng.py::test_the_protocol_end_to_end for the same quantity."""
    from mcmc_spec_amd.sampler import run_reference_protocol
    want, wfiles, _ = protocol_reference(nw, tmp_path_factory)
    dev = device(nw, autocorr=autocorr)
    got = run_reference_protocol(dev, tight_p0(nw), nburn=7, nsteps=40, nthin=10, dirname=str(tmp_path))
    assert got.shape == want.shape == (nw * 40, NDIM) and np.array_equal(got, want)
    assert dev._drawn == 47
    gfiles = _files(str(tmp_path))
    assert sorted(gfiles) == sorted(wfiles) and 'samples.txt' in wfiles and 'run_autocorr.txt' in wfiles
    assert 'run_0_burnin.txt' in wfiles and 'run_30_results.txt' in wfiles
    for name in wfiles:
        if autocorr == 'host' or name != 'run_autocorr.txt':
            assert gfiles[name] == wfiles[name], name
            continue
        g, w = (np.array([float(v) for v in x[name].split()]) for x in (gfiles, wfiles))
        print('autocorr lines, {} walkers: device {} host {} rel {}'.format(nw, g, w, np.abs(g - w) / np.abs(w)))
        assert g.shape == w.shape == (4,) and np.isnan(g[0]) and np.isnan(w[0])     # checks at n = 0, 10, 20, 30
        assert np.all(np.isfinite(w[1:]))
        for i in (1, 2, 3):
            assert np.isclose(g[i], w[i], rtol=1e-9, atol=0), (i, g[i], w[i])


# ---- 5. a loop left early ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nw', ENSEMBLES)
def test_a_loop_left_early_leaves_the_stream_past_what_was_queued(nw):
    """sample(p0, iterations=20) left after 3 iterations: the chunk pipeline keeps two chunks in flight -- chunk 0 is
    collected (and its rows yielded) only after chunk 1 has been queued -- so 2 chunks x 4 = 8 iterations of the stream
    are spent, 3 of them seen.  The next run goes on from 8."""
    queued = 2 * CHUNK
    dev = device(nw)
    for n, _ in enumerate(dev.sample(p0_of(nw), iterations=20)):
        if n == 2:
            break
    assert dev.iteration == 3 and dev._drawn == queued
    st = dev.get_last_sample()
    es = twin(nw)
    hs = es.run_mcmc(p0_of(nw), 3)
    assert np.array_equal(dev.get_chain(), es.get_chain()) and np.array_equal(st.coords, hs.coords) and np.array_equal(st.log_prob, hs.log_prob)
    assert es._drawn == 3
    es._drawn = queued
    dev.reset()
    es.reset()
    ds = dev.run_mcmc(st, 5)
    same(dev, ds, Snap(es, es.run_mcmc(hs, 5)))
    assert dev._drawn == queued + 5


# ---- 6. sharded, world 1 --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('nw', ENSEMBLES)
def test_a_sharded_run_of_one_rank_walks_the_unsharded_chain(nw):
    first, second = reference(nw, False)
    dev = device(nw, shard=(0, 1))
    st = dev.run_mcmc(p0_of(nw), 5)
    same(dev, st, first)
    st = dev.run_mcmc(st, 6)
    assert dev.overlapped is False and dev._drawn == 11
    same(dev, st, second)


# ---- 7. refusals through the ABI, mixed chunks ------------------------------------------------------------------------------------
@pytest.mark.parametrize('nw', ENSEMBLES)
def test_refusals_through_the_abi_and_mixed_chunks(nw):
    from mcmc_spec_amd import _lib
    eng, _ = _config2()
    ctx = eng.ctx
    first, _ = reference(nw, False)
    p0 = p0_of(nw)
    lp0 = eng.logposterior(p0)
    fed = ctx.sampler_draw(SEED, A, 0, 2, nw, NDIM)     # (the generator's own numbers for iterations 0 and 1)
    ctx.sampler_policy(-1)
    ctx.sampler_begin(_lib.MODE_LOGPOST, p0, lp0, 2)
    try:
        for kw in (dict(a=1.0, first_iter=0), dict(a=float('nan'), first_iter=0), dict(a=A, first_iter=-1)):
            with pytest.raises(_lib.MsxError) as ei:
                ctx.sampler_enqueue_drawn(0, 2, SEED, **kw)
            assert ei.value.code == _lib.MSX_ERR_INVALID, kw
        with pytest.raises(_lib.MsxError) as ei:   # (the chunk length is checked as the host-fed entry checks it)
            ctx.sampler_enqueue_drawn(0, 3, SEED, A, 0)
        assert ei.value.code == _lib.MSX_ERR_INVALID
        # nothing was queued: the slot is free and the run takes a valid chunk, then the next one
        ctx.sampler_enqueue_drawn(0, 2, SEED, A, 0)
        ctx.sampler_enqueue_drawn(1, 2, SEED, A, 2)
        with pytest.raises(_lib.MsxError, match='not collected'):
            ctx.sampler_enqueue_drawn(0, 2, SEED, A, 4)
        drawn = [ctx.sampler_collect(s, 2) for s in (0, 1)]
    finally:
        ctx.sampler_end()
    assert drawn[0][3] == 0 and drawn[1][3] == 0
    # ... and ran as usual: iterations 0..3 of the twin's chain
    assert np.array_equal(np.concatenate([drawn[0][0], drawn[1][0]]), first.chain[:4])
    assert np.array_equal(np.concatenate([drawn[0][1], drawn[1][1]]), first.logp[:4])

    # a host-fed chunk for iterations 0..1, then a drawn one from iteration 2, in one run: the all-drawn run
    ctx.sampler_begin(_lib.MODE_LOGPOST, p0, lp0, 2)
    try:
        ctx.sampler_enqueue(0, *fed)
        ctx.sampler_enqueue_drawn(1, 2, SEED, A, 2)
        mixed = [ctx.sampler_collect(s, 2) for s in (0, 1)]
    finally:
        coords, logp = ctx.sampler_end(want_state=True)
    for d, m in zip(drawn, mixed):
        assert np.array_equal(d[0], m[0]) and np.array_equal(d[1], m[1]) and np.array_equal(d[2], m[2]) and m[3] == 0
    assert np.array_equal(coords, drawn[1][0][-1]) and np.array_equal(logp, drawn[1][1][-1])
    assert 0 < drawn[1][2].sum() < 4 * nw


# ---- 8. seed forms ------------------------------------------------------------------------------------------------------------------
def test_a_seed_sequence_keys_the_stream_by_its_derived_value():
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    eng, _ = _config2()
    nw = 18
    key = int(np.random.SeedSequence(9).generate_state(1, dtype=np.uint64)[0])
    host_drawn = DeviceEnsembleSampler(nw, NDIM, eng, seed=np.random.SeedSequence(9), chunk=CHUNK)
    assert host_drawn.device_seed is None
    host_drawn.run_mcmc(p0_of(nw), 2)
    assert host_drawn._drawn == 0 and host_drawn.get_chain().shape == (2, nw, NDIM)
    dev = device(nw, seed=np.random.SeedSequence(9))
    assert dev.device_seed == key
    st = dev.run_mcmc(p0_of(nw), 5)
    st = dev.run_mcmc(st, 6)
    es = twin(nw, key)
    hs = es.run_mcmc(p0_of(nw), 5)
    same(dev, st, Snap(es, es.run_mcmc(hs, 6)))
    assert not np.array_equal(dev.get_chain(), reference(nw, False)[1].chain)
