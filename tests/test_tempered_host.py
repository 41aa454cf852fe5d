"""CPU: parallel tempering on the host (mcmc_spec_amd.tempered): the host loop against a plain-Python
restatement (tests/tempered_numpy.py), one rung against the ensemble sampler, the swap draws' counter stream, what every
rung samples, the mode weights of a bimodal target, the refusals, and what ``DeviceTemperedSampler`` asks of a context (a
recording one: no library, no GPU)."""
import numpy as np
import pytest

import common  # noqa: F401
import tempered_numpy as tn
from mcmc_spec_amd import tempered
from mcmc_spec_amd.moves import DEMove, StretchMove, counter_draws_moves, parse_moves
from mcmc_spec_amd.sampler import EnsembleSampler, device_seed
from mcmc_spec_amd.tempered import DeviceTemperedSampler, TemperedSampler, TemperedState, default_betas
from test_sampler_rng_abi import mix64

BETAS3 = [1.0, 0.5, 0.25]


def mix():
    return [(StretchMove(), 0.5), (DEMove(), 0.4), (DEMove(gamma0=1.0), 0.1)]


def box(half):
    return lambda x: np.where(np.all(np.abs(x) < half, axis=-1), 0.0, -np.inf)


def tilted(x):   # a tilted Gaussian likelihood
    return -0.5 * np.sum((x - 0.3) ** 2 * np.arange(1, x.shape[-1] + 1), axis=-1)


def gauss(x):
    return -0.5 * np.sum(x * x, axis=-1)


def start(nw, ndim, seed=4, scale=1.0):
    return scale * np.random.default_rng(seed).uniform(-1.0, 1.0, size=(nw, ndim))


# ---- 1. the host loop on its own draws, against the plain-Python restatement ----------------------------------------------
def test_the_host_loop_is_the_plain_restatement_bit_for_bit():
    T, nw, ndim, m = 3, 12, 3, 9
    prior = box(2.5)                       # proposals leave the box: -inf, and -inf - -inf = nan on a rejected pair
    p0 = start(nw, ndim, scale=2.0)
    s = TemperedSampler(nw, ndim, tilted, prior, betas=BETAS3, seed=21, moves=mix())
    s.run_mcmc(p0, m)
    twin = TemperedSampler(nw, ndim, tilted, prior, betas=BETAS3, seed=21, moves=mix())    # (its generators only)
    coords = np.repeat(p0[None], T, axis=0).copy()
    ll, lpr = tilted(coords), prior(coords)
    nacc, nswap = np.zeros((T, nw)), np.zeros(T - 1, dtype=np.int64)
    _count.inf = 0
    for i in range(m):
        members, swap_logu = twin._draw_steps(1)
        one = [tuple(a[0] for a in mem) for mem in members]
        nacc += tn.iterate(BETAS3, coords, ll, lpr, tilted, lambda q: _count(prior(q)), one)
        nswap += tn.sweep(BETAS3, coords, ll, lpr, swap_logu[0])
        assert np.array_equal(s.get_chain(t=None)[i], coords), i
        assert np.array_equal(s.get_log_like(t=None)[i], ll) and np.array_equal(s.get_log_prior(t=None)[i], lpr), i
    assert _count.inf > 0                                       # the -inf branch was walked
    assert np.array_equal(s.acceptance_fraction, nacc / m) and 0.1 < nacc.mean() / m < 0.9
    assert np.array_equal(s.swap_fraction, nswap / (m * nw))
    assert np.all(nswap > 0) and np.all(nswap < m * nw)               # swaps both happened and were refused
    assert np.array_equal(s.get_log_prob(0), s.get_log_prior(0) + s.get_log_like(0))
    assert s.get_chain().shape == (m, nw, ndim) and s.get_chain(flat=True).shape == (m * nw, ndim)
    assert s.get_chain(t=None, flat=True).shape == (T, m * nw, ndim) and s.get_chain(t=2, thin=2, discard=1).shape == (4, nw, ndim)
    last = s.get_last_sample()
    assert isinstance(last, TemperedState) and np.array_equal(last.coords, coords) and np.array_equal(last.log_like, ll)
    # m iterations drawn at once are m draws of one: the device sampler's chunks are the host loop's iterations
    a, b = (TemperedSampler(nw, ndim, tilted, prior, betas=BETAS3, seed=21, moves=mix()) for _ in range(2))
    whole = a._draw_steps(4)
    for i in range(4):
        mem, sw = b._draw_steps(1)
        assert np.array_equal(sw[0], whole[1][i])
        assert all(np.array_equal(x[0], y[i]) for t in range(T) for x, y in zip(mem[t], whole[0][t]))


def _count(v):
    _count.inf += int(np.count_nonzero(np.isneginf(v)))
    return v


_count.inf = 0


# ---- 2. nothing to temper -----------------------------------------------------------------------------------------------------
def test_one_rung_is_the_ensemble_sampler_on_the_posterior():
    nw, ndim, m = 12, 3, 25
    prior = box(2.5)
    p0 = start(nw, ndim, scale=2.0)
    s = TemperedSampler(nw, ndim, tilted, prior, betas=[1.0], seed=33, moves=mix())
    assert s.seeds == [33] and s.ntemps == 1
    s.run_mcmc(p0, m)
    e = EnsembleSampler(nw, ndim, lambda x: prior(x) + tilted(x), vectorize=True, seed=s.seeds[0], moves=mix(), _general=True)
    e.run_mcmc(p0, m)
    assert np.array_equal(s.get_chain(), e.get_chain()) and np.array_equal(s.get_log_prob(), e.get_log_prob())   # 1.0 * ll is exact
    assert np.array_equal(s.acceptance_fraction[0], e.acceptance_fraction) and s.swap_fraction.shape == (0,)
    assert TemperedSampler(nw, ndim, tilted, prior, ntemps=1).betas.tolist() == [1.0]


# ---- 3. the streams ---------------------------------------------------------------------------------------------------------------
def test_the_rungs_streams_are_the_moves_streams_and_the_swap_stream_is_its_own():
    seeds, nw, ndim = [2**63 + 5, 17, 2**64 - 1], 18, 6
    members, swap_logu = tempered.counter_draws_tempered(seeds, mix(), ndim, 3, 7, nw)
    for t, s in enumerate(seeds):
        want = counter_draws_moves(s, mix(), ndim, 3, 7, nw)
        assert len(members[t]) == 8 and all(np.array_equal(a, b) for a, b in zip(members[t], want))
    # the swap draws in Python integers; a later chunk is the stream's later rows
    assert swap_logu.shape == (7, 2, nw)
    assert np.allclose(swap_logu, tn.swap_logu_int(seeds[0], 3, 7, 3, nw), rtol=4e-16, atol=0)
    whole = tempered.counter_swap_logu(seeds[0], 0, 10, 3, nw)
    assert np.array_equal(whole[3:], swap_logu)
    assert tempered.counter_swap_logu(5, 0, 2, 1, nw).shape == (2, 0, nw)
    # the defaults: seeds[t] = (device_seed(seed) + t) mod 2^64
    assert tempered.resolve_seeds(3, 2**64 - 2, None) == [2**64 - 2, 2**64 - 1, 0]
    assert tempered.resolve_seeds(2, [1, 2, 3], None) == [device_seed([1, 2, 3]), (device_seed([1, 2, 3]) + 1) % 2**64]


def test_no_two_of_the_fifteen_fields_alias():
    """Streams 0..13 as tests/test_moves_host.py lists them, and stream 14's (iteration, pair, walker) fields for every pair
    index 0..63 and walker 0..4095, over 8 iterations: pairwise distinct counters and outputs, every index inside the
    field's 24 bits, every stream inside its 4."""
    seed, nw, its = 2024, 4096, np.arange(8)[:, None]
    sizes = {0: nw, 7: 1, 14: 64 * tempered.SWAP_STRIDE}
    ctrs, keys = [], []
    for stream in range(15):
        assert stream < 1 << 4
        idx = np.arange(sizes.get(stream, nw // 2))[None, :]
        assert int(idx.max()) < 1 << 24
        ctrs.append(((its.astype(np.uint64) << np.uint64(28)) + (np.uint64(stream) << np.uint64(24)) + idx.astype(np.uint64)).ravel())
        keys.append(mix64(seed, its, stream, idx).ravel())
    ctrs, keys = np.concatenate(ctrs), np.concatenate(keys)
    assert len(keys) == 8 * (nw + 1 + 12 * (nw // 2) + 64 * 4096)
    assert len(np.unique(ctrs)) == len(ctrs) and len(np.unique(keys)) == len(keys)
    assert tempered.SWAP_STREAM == tn.SWAP_STREAM == 14 and tempered.SWAP_STRIDE == tn.SWAP_STRIDE == 4096
    top = 63 * 4096 + 4095                                                    # the largest index
    assert top < 1 << 24 and tn.swap_index(63, 4095) == 62 * 4096 + 4095 <= top
    assert int(mix64(seed, np.array([5]), 14, np.array([top]))[0]) == tn.mix64_int(seed, 5, 14, top)
    # (iteration, pair, walker) -> counter is injective: the index packs pair and walker without overlap
    assert len({tn.swap_index(t, w) for t in (1, 2, 63) for w in (0, 1, 4095)}) == 9
    # the largest ladder through the restatement under test
    got = tempered.counter_swap_logu(seed, 4, 2, 64, 4096)
    assert got.shape == (2, 63, 4096) and np.isclose(got[1, 62, 4095], np.log(tn.swap_uniform_int(seed, 5, 63, 4095)), rtol=4e-16, atol=0)


# ---- 4. what every rung samples --------------------------------------------------------------------------------------------------
def test_each_rung_samples_its_own_density():
    """Likelihood N(0, I_3) under a flat box |x_i| < 50, betas 1, 0.5, 0.25: rung t's variance is 1 / beta_t.  40 walkers
    started at 0 +- 0.1, 4,000 iterations, the first 1,000 discarded: every |mean| <= 0.1 sigma_t and every variance within
    +-10 % (the bounds of test_stationarity_on_a_unit_gaussian).  The restatement's own run (tempered_numpy.run) gave
    <= 0.027 sigma_t and [0.951, 1.023] over 10 seeds at this length, this sampler <= 0.036 and [0.977, 1.031]; swap
    fractions 0.58-0.59.  A wrong swap rule -- a wrong sign, beta for the difference of the betas, coordinates swapped
    without their values -- leaves the rungs with each other's variances."""
    n, nw = 4000, 40
    s = TemperedSampler(nw, 3, gauss, box(50.0), betas=BETAS3, seed=3)
    s.run_mcmc(0.1 * np.random.default_rng(1).normal(size=(nw, 3)), n)
    c = s.get_chain(t=None, discard=n // 4)
    for t, beta in enumerate(BETAS3):
        f = c[:, t].reshape(-1, 3)
        mean, var = f.mean(axis=0) * np.sqrt(beta), f.var(axis=0) * beta
        print('rung', t, 'max |mean| / sigma', np.abs(mean).max(), 'variance x beta', var.min(), var.max())
        assert np.all(np.abs(mean) <= 0.1) and np.all(var >= 0.9) and np.all(var <= 1.1)
    print('swap fractions', s.swap_fraction)
    assert np.all(s.swap_fraction > 0.3) and np.all(s.swap_fraction < 0.9)


# ---- 5. mode weights ----------------------------------------------------------------------------------------------------------------
def bimodal(x):
    """Two unit Gaussians in 6-D, 10 sigma apart along x0 (at -5 and +5), weights 0.8 / 0.2 (tests/test_moves_host.py), here
    as the likelihood under the box prior |x_i| < 20."""
    r2 = np.sum(x[..., 1:] ** 2, axis=-1)
    return np.logaddexp(np.log(0.8) - 0.5 * ((x[..., 0] + 5.0) ** 2 + r2), np.log(0.2) - 0.5 * ((x[..., 0] - 5.0) ** 2 + r2))


def test_mode_weights_of_a_bimodal_target():
    """50 walkers started 25 / 25, default_betas(6, 0.02), the stretch move, 3,000 iterations, the second half counted: the
    cold rung's x0 < 0 fraction lies in 0.75..0.85 for the true 0.8 and every adjacent swap fraction in 0.2..0.55.  This
    sampler over seeds 0..9: 0.783-0.824, swap fractions 0.346-0.397 (the specification's experiment: 0.796-0.813 over 6
    seeds, 0.35-0.39; the stretch move alone leaves 0.47-0.60)."""
    p0 = np.random.default_rng(2).normal(size=(50, 6))
    p0[:25, 0] -= 5.0
    p0[25:, 0] += 5.0
    s = TemperedSampler(50, 6, bimodal, box(20.0), betas=default_betas(6, 0.02), seed=5)
    s.run_mcmc(p0, 3000)
    heavy = float(np.mean(s.get_chain(discard=1500, flat=True)[:, 0] < 0.0))
    print('x0 < 0 fraction of the cold rung', heavy, ' swap fractions', s.swap_fraction)
    assert 0.75 <= heavy <= 0.85
    assert np.all(s.swap_fraction >= 0.2) and np.all(s.swap_fraction <= 0.55)


# ---- 6. refusals ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('kw', [dict(betas=[1.0, 0.5, 0.5]), dict(betas=[0.5, 1.0]), dict(betas=[1.0, 0.0]), dict(betas=[1.0, -0.5]),
                                dict(betas=[1.0, float('nan')]), dict(betas=[float('inf'), 1.0]), dict(ntemps=65), dict(ntemps=0),
                                dict(betas=np.geomspace(1.0, 0.01, 65)), dict(ntemps=3, betas=[1.0, 0.5]), dict(), dict(betas=[])],
                         ids=['equal', 'ascending', 'zero', 'negative', 'nan', 'inf', '65', '0', '65 betas', 'inconsistent', 'neither', 'empty'])
def test_refusals_raise_value_error(kw):
    with pytest.raises(ValueError):
        TemperedSampler(12, 3, gauss, box(5.0), **kw)
    with pytest.raises(ValueError):
        DeviceTemperedSampler(16, 6, TemperedEngine(), **kw)


def test_more_refusals():
    with pytest.raises(ValueError):
        TemperedSampler(13, 3, gauss, box(5.0), betas=BETAS3)                    # odd
    with pytest.raises(ValueError):
        DeviceTemperedSampler(15, 6, TemperedEngine(), betas=BETAS3)
    with pytest.raises(ValueError):
        TemperedSampler(12, 3, gauss, box(5.0), betas=BETAS3, seeds=[1, 2])      # one seed per rung
    with pytest.raises(ValueError):
        DeviceTemperedSampler(16, 6, TemperedEngine(), betas=BETAS3, rng='gpu')
    p0 = start(12, 3)
    p0[5, 1] = 7.0                                                               # outside the prior
    with pytest.raises(ValueError, match='prior'):
        TemperedSampler(12, 3, gauss, box(5.0), betas=BETAS3, seed=1).run_mcmc(p0, 2)
    with pytest.raises(ValueError):
        TemperedSampler(12, 3, gauss, box(5.0), betas=BETAS3, seed=1).run_mcmc(start(10, 3), 2)
    with pytest.raises(ValueError, match='NaN'):
        TemperedSampler(12, 3, lambda x: np.full(len(x), np.nan), box(5.0), betas=BETAS3, seed=1).run_mcmc(start(12, 3), 2)
    ok = TemperedSampler(12, 3, gauss, box(5.0), ntemps=3, betas=BETAS3)
    assert ok.betas.tolist() == BETAS3
    assert np.array_equal(TemperedSampler(12, 3, gauss, box(5.0), ntemps=6, beta_min=0.02).betas, default_betas(6, 0.02))
    assert np.array_equal(default_betas(6, 0.02), np.geomspace(1.0, 0.02, 6))
    assert ok._moves.pure_stretch and parse_moves(mix()).kinds == TemperedSampler(12, 3, gauss, box(5.0), ntemps=2, moves=mix())._moves.kinds


def test_statuses_follow_the_rule():
    """A proposal the prior rejects (status 1) is rejected whatever its likelihood reports; an error status of the likelihood
    on a proposal the prior admits, and one of the prior, raise."""
    def prior(q):
        out = box(2.0)(q)
        return out, np.where(np.isfinite(out), 0, 1).astype(np.int32)

    def like_err_outside(q):   # KeyError status wherever the prior rejects: ignored
        inside = np.all(np.abs(q) < 2.0, axis=-1)
        return np.where(inside, gauss(q), np.nan), np.where(inside, 0, 2).astype(np.int32)

    def plain_like(q):
        return gauss(q), np.zeros(len(q), dtype=np.int32)

    p0 = start(12, 3, scale=1.9)
    a = TemperedSampler(12, 3, like_err_outside, prior, betas=BETAS3, seed=8)
    b = TemperedSampler(12, 3, plain_like, prior, betas=BETAS3, seed=8)
    a.run_mcmc(p0, 30), b.run_mcmc(p0, 30)
    assert np.array_equal(a.get_chain(t=None), b.get_chain(t=None)) and np.all(np.abs(a.get_chain(t=None)) < 2.0)
    assert np.any(a.acceptance_fraction < 1.0)

    def like_err_inside(q):
        return gauss(q), np.full(len(q), 3, dtype=np.int32)
    with pytest.raises(IndexError):
        TemperedSampler(12, 3, like_err_inside, prior, betas=BETAS3, seed=8).run_mcmc(p0, 3)
    with pytest.raises(ValueError, match='interpolation'):
        TemperedSampler(12, 3, plain_like, lambda q: (np.zeros(len(q)), np.full(len(q), 4, dtype=np.int32)), betas=BETAS3).run_mcmc(p0, 3)


# ---- 7. what DeviceTemperedSampler asks of a context ----------------------------------------------------------------------------
class TemperedContext:
    """Every call recorded; chunks 'run' by leaving the walkers where they are.  (No library, no GPU.)"""

    def __init__(self):
        self.calls, self.pending = [], {}

    def logprob_batch(self, q, mode):
        return np.zeros(len(q)), np.zeros(len(q), dtype=np.int32)

    def sampler_policy(self, overlap):
        self.calls.append(('policy', overlap))

    def tempered_begin(self, betas, coords, ll, lpr, chunk):
        self.calls.append(('begin', np.array(betas), chunk))
        self.state = coords.copy(), ll.copy(), lpr.copy()

    def tempered_enqueue_drawn(self, slot, nsteps, seeds, moves, first_iter):
        assert slot not in self.pending, 'slot not collected yet'
        self.calls.append(('drawn', slot, nsteps, list(seeds), moves, first_iter))
        self.pending[slot] = nsteps
        return nsteps

    def tempered_enqueue(self, slot, *arrays):
        assert slot not in self.pending, 'slot not collected yet'
        self.calls.append(('fed', slot, arrays))
        self.pending[slot] = len(arrays[2])
        return len(arrays[2])

    def tempered_collect(self, slot, nsteps):
        assert self.pending.pop(slot) == nsteps
        self.calls.append(('collect', slot, nsteps))
        c, ll, lpr = self.state
        T, nw, _ = c.shape
        return (np.broadcast_to(c, (nsteps,) + c.shape).copy(), np.broadcast_to(ll, (nsteps, T, nw)).copy(),
                np.broadcast_to(lpr, (nsteps, T, nw)).copy(), np.zeros((T, nw), dtype=np.int64), np.zeros(T - 1, dtype=np.int64),
                np.zeros(T, dtype=np.int32))

    def tempered_end(self, want_state=False):
        self.calls.append(('end',))
        self.pending.clear()


class TemperedEngine:
    def __init__(self):
        self.ctx = TemperedContext()


def test_the_device_sampler_queues_chunks_at_the_absolute_iteration():
    """Runs of 5 and 6 iterations at chunk = 4: chunks of 4 + 1 and 4 + 2, first iterations 0, 4 | 5, 9; reset() leaves the
    position alone; a slot is collected before it is reused; end is called when a consumer breaks out."""
    eng = TemperedEngine()
    s = DeviceTemperedSampler(16, 6, eng, betas=BETAS3, seed=11, chunk=4, rng='device', moves=mix())
    assert s.seeds == [11, 12, 13]
    st = s.run_mcmc(np.random.default_rng(0).normal(size=(16, 6)), 5)
    assert s._drawn == 5 and isinstance(st, TemperedState) and st.coords.shape == (3, 16, 6)
    s.reset()
    assert s._drawn == 5 and s.iteration == 0 and s.get_chain().shape[0] == 0
    s.run_mcmc(st, 6)
    assert s._drawn == 11 and s.get_chain().shape == (6, 16, 6) and s.get_chain(t=None).shape == (6, 3, 16, 6)
    calls = eng.ctx.calls
    drawn = [c for c in calls if c[0] == 'drawn']
    assert [c[5] for c in drawn] == [0, 4, 5, 9] and [c[2] for c in drawn] == [4, 1, 4, 2] and [c[1] for c in drawn] == [0, 1, 0, 1]
    assert all(c[3] == [11, 12, 13] and c[4] is s._moves and len(c[4]) == 3 for c in drawn)
    names = [c[0] for c in calls]
    assert names.count('begin') == 2 and names.count('end') == 2 and names.count('policy') == 2
    assert [c for c in calls if c[0] == 'policy'] == [('policy', 0)] * 2 and names.index('policy') < names.index('begin')
    assert np.array_equal(calls[names.index('begin')][1], BETAS3) and calls[names.index('begin')][2] == 4
    # a consumer that breaks out: the run is ended, and the position counts the chunks QUEUED
    eng2 = TemperedEngine()
    s2 = DeviceTemperedSampler(16, 6, eng2, betas=BETAS3, seed=11, chunk=4, rng='device')
    for i, _ in enumerate(s2.sample(st, iterations=20)):
        if i == 1:
            break
    assert [c[0] for c in eng2.ctx.calls][-1] == 'end' and s2._drawn == 8 and s2.iteration == 2
    # with three chunks in a run, slot 0 is collected before its second chunk is queued
    eng3 = TemperedEngine()
    DeviceTemperedSampler(16, 6, eng3, betas=BETAS3, seed=11, chunk=4, rng='device').run_mcmc(st, 12)
    seq = [(c[0], c[1]) for c in eng3.ctx.calls if c[0] in ('drawn', 'collect')]
    assert seq == [('drawn', 0), ('drawn', 1), ('collect', 0), ('drawn', 0), ('collect', 1), ('collect', 0)]


def test_the_host_drawn_device_sampler_uploads_the_twins_draws():
    eng = TemperedEngine()
    s = DeviceTemperedSampler(16, 6, eng, betas=BETAS3, seed=11, chunk=4, moves=mix())
    s.run_mcmc(np.zeros((16, 6)), 6)
    chunks = [c[2] for c in eng.ctx.calls if c[0] == 'fed']
    assert [len(a[2]) for a in chunks] == [4, 2] and all(len(a) == 9 for a in chunks)
    assert chunks[0][0].shape == (4, 3, 2, 8) and chunks[0][2].shape == (4, 3) and chunks[0][8].shape == (4, 2, 16)
    twin = TemperedSampler(16, 6, gauss, box(5.0), betas=BETAS3, seed=11, moves=mix())
    members, swap_logu = twin._draw_steps(6)
    for i in range(8):
        got = np.concatenate([a[i] for a in chunks])
        assert all(np.array_equal(got[:, t], members[t][i]) for t in range(3)), i
    assert np.array_equal(np.concatenate([a[8] for a in chunks]), swap_logu)
    assert not [c for c in eng.ctx.calls if c[0] == 'drawn']
