"""CPU: the single-target device-drawn sampler's stream position (include/msx.h, msx_sampler_enqueue_drawn's first_iter;
mcmc_spec_amd.sampler.DeviceEnsembleSampler(rng='device')): the entry point is declared, exported and mirrored with the
absolute first iteration; the constructor derives the generator's key only for rng='device', by the one function the group
sampler uses, and refuses a sharded run that would draw per-rank entropy; the position passed to the library goes on across
runs and reset(); and the counter stream itself -- restated here in plain integer arithmetic -- neither aliases across its
fields nor correlates between neighbouring iterations or seeds.  No compute calls (no GPU here)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import common  # noqa: F401
from mcmc_spec_amd import _lib
from mcmc_spec_amd.group import DeviceGroupSampler
from mcmc_spec_amd.sampler import DeviceEnsembleSampler, State, counter_draws, device_seed
from test_group_rng_abi import StubGroup

ROOT = common.ROOT
HDR = os.path.join(ROOT, 'include', 'msx.h')
NAME = 'msx_sampler_enqueue_drawn'
NDIM = 6
M64 = 0xffffffffffffffff


# ---- 1. the ABI ------------------------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_first_iteration():
    import __graft_entry__ as ge
    ge.build()
    txt = re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)
    m = re.search(r'\bint ' + NAME + r'\s*\(([^)]*)\)\s*;', txt)
    assert m, NAME
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    assert params == ['msx_ctx *ctx', 'int32_t slot', 'int64_t nsteps', 'uint64_t seed', 'double a', 'int64_t first_iter'], params
    lib = _lib.load()
    assert NAME in _lib.EXPORTED
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.c_double, C.c_int64]
    import inspect
    assert list(inspect.signature(_lib.Context.sampler_enqueue_drawn).parameters) == ['self', 'slot', 'nsteps', 'seed', 'a', 'first_iter']


# ---- 2. the constructor, before anything touches a GPU -----------------------------------------------------------------
class RecordingContext:
    """What DeviceEnsembleSampler.sample asks of a context: every call recorded, chunks 'run' by leaving the walkers where
    they are.  (No library, no GPU.)"""

    def __init__(self, nw, ndim):
        self.nw, self.ndim = nw, ndim
        self.calls = []
        self.pending = {}

    def sampler_policy(self, overlap):
        self.calls.append(('policy', overlap))

    def sampler_begin(self, mode, coords, logp, chunk):
        self.calls.append(('begin', chunk))
        self.coords, self.logp = coords.copy(), logp.copy()

    def sampler_shard(self, rank, world):
        self.calls.append(('shard', rank, world))

    def sampler_enqueue_drawn(self, slot, nsteps, seed, a, first_iter):
        assert slot not in self.pending, 'slot not collected yet'
        self.calls.append(('drawn', slot, nsteps, seed, a, first_iter))
        self.pending[slot] = nsteps
        return nsteps

    def sampler_enqueue(self, slot, *arrays):
        raise AssertionError("rng='device' draws nothing on the host")

    def sampler_overlapped(self):
        return 0

    def sampler_collect(self, slot, nsteps):
        assert self.pending.pop(slot) == nsteps
        self.calls.append(('collect', slot, nsteps))
        return (np.broadcast_to(self.coords, (nsteps, self.nw, self.ndim)).copy(),
                np.broadcast_to(self.logp, (nsteps, self.nw)).copy(), np.zeros(self.nw, dtype=np.int64), 0)

    def sampler_end(self, want_state=False):
        self.calls.append(('end',))
        self.pending.clear()

    def first_iters(self):
        return [c[5] for c in self.calls if c[0] == 'drawn']


class StubEngine:
    """What DeviceEnsembleSampler reads of an Engine."""

    def __init__(self, nw=16, ndim=NDIM):
        self.ctx = RecordingContext(nw, ndim)

    def logposterior(self, theta):
        return np.zeros(len(theta))

    loglikelihood = logposterior


def _ss_key(entropy):
    return int(np.random.SeedSequence(entropy).generate_state(1, dtype=np.uint64)[0])


SEED_FORMS = [(7, 7), (2**64 + 5, 5), (2**63 + 41, 2**63 + 41), (np.int64(12), 12), (np.random.SeedSequence(9), _ss_key(9)),
              ([1, 2, 3], _ss_key([1, 2, 3])), (None, None)]


@pytest.mark.parametrize('seed,key', SEED_FORMS, ids=['int', 'int>=2^64', 'int>=2^63', 'np.int64', 'SeedSequence', 'list', 'None'])
def test_constructor_takes_every_seed_form_with_either_rng(seed, key):
    host = DeviceEnsembleSampler(16, NDIM, StubEngine(), seed=seed)
    assert host.rng_mode == 'host' and host.device_seed is None
    dev = DeviceEnsembleSampler(16, NDIM, StubEngine(), seed=seed, rng='device')
    assert dev.rng_mode == 'device' and isinstance(dev.device_seed, int) and 0 <= dev.device_seed < 2**64
    if key is not None:
        assert dev.device_seed == key == device_seed(seed)
        # ... which is what the group sampler derives for a target of that seed: one function
        grp = DeviceGroupSampler([16], NDIM, StubGroup(1), seeds=[seed], rng='device')
        assert grp.device_seeds == [key]


def test_fresh_entropy_differs_between_samplers_and_is_refused_where_ranks_must_agree():
    a, b = (DeviceEnsembleSampler(16, NDIM, StubEngine(), rng='device').device_seed for _ in range(2))
    assert a != b
    with pytest.raises(ValueError, match='seed'):
        DeviceEnsembleSampler(16, NDIM, StubEngine(), rng='device', shard=(1, 2))
    # what is still taken: world 1, an explicit seed, and host draws (whose None seed was always the caller's affair)
    assert DeviceEnsembleSampler(16, NDIM, StubEngine(), rng='device', shard=(0, 1)).device_seed is not None
    assert DeviceEnsembleSampler(16, NDIM, StubEngine(), rng='device', shard=(1, 2), seed=3).device_seed == 3
    assert DeviceEnsembleSampler(16, NDIM, StubEngine(), shard=(1, 2)).device_seed is None


# ---- 3. the position passed to the library ----------------------------------------------------------------------------
def test_first_iterations_over_two_runs_and_a_reset():
    """Runs of 5 and 6 iterations at chunk = 4: chunks of 4 + 1 and 4 + 2, first iterations 0, 4 | 5, 9."""
    eng = StubEngine()
    s = DeviceEnsembleSampler(16, NDIM, eng, seed=11, chunk=4, rng='device')
    p0 = np.random.default_rng(0).normal(size=(16, NDIM))
    st = s.run_mcmc(State(p0, np.zeros(16)), 5)
    assert s._drawn == 5 and s.iteration == 5
    s.reset()
    assert s._drawn == 5 and s.iteration == 0
    s.run_mcmc(st, 6)
    assert s._drawn == 11 and s.get_chain().shape == (6, 16, NDIM)
    drawn = [c for c in eng.ctx.calls if c[0] == 'drawn']
    assert eng.ctx.first_iters() == [0, 4, 5, 9]
    assert [c[2] for c in drawn] == [4, 1, 4, 2]
    assert all(c[3] == 11 and c[4] == 2.0 for c in drawn)
    assert [c[0] for c in eng.ctx.calls].count('begin') == 2 == [c[0] for c in eng.ctx.calls].count('end')


def test_the_position_counts_iterations_queued_when_a_loop_is_left_early():
    """_pump keeps two chunks in flight: chunk 0 is collected only after chunk 1 has been queued, so a loop left inside
    chunk 0 (3 < 4 iterations) has queued 2 chunks = 8 iterations."""
    eng = StubEngine()
    s = DeviceEnsembleSampler(16, NDIM, eng, seed=11, chunk=4, rng='device')
    p0 = State(np.zeros((16, NDIM)), np.zeros(16))
    for n, _ in enumerate(s.sample(p0, iterations=20)):
        if n == 2:
            break
    assert s.iteration == 3 and s._drawn == 8 and eng.ctx.first_iters() == [0, 4]
    assert eng.ctx.calls[-1] == ('end',)
    s.run_mcmc(p0, 1)
    assert eng.ctx.first_iters() == [0, 4, 8]


# ---- 4. the stream itself, in plain arithmetic --------------------------------------------------------------------------
# counter = (it << 28) + (stream << 24) + index: the index has 24 bits (up to 4096 walkers are drawn: 12), the stream 4
# (7 are used: 0 the split's keys, 1..3 and 4..6 the two half-steps' u_z, u_p, u_a), the iteration the remaining 36 before
# the sum wraps at 2^64 -- 6.8e10 iterations.  Within those widths the three fields cannot alias.
IDX_BITS, STREAM_BITS, IT_BITS = 24, 4, 36


def mix64_int(seed, it, stream, index):
    """SplitMix64's output function over the counter sequence, in Python integers."""
    assert index < 1 << IDX_BITS and stream < 1 << STREAM_BITS and it < 1 << IT_BITS
    ctr = (it << 28) + (stream << 24) + index
    x = ((seed & M64) * 0xD1342543DE82EF95 + (ctr + 1) * 0x9E3779B97F4A7C15) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    return x


def mix64(seed, it, stream, index):
    """The same over arrays (uint64 wraps like the masks above; checked against mix64_int below)."""
    u = np.uint64
    with np.errstate(over='ignore'):
        ctr = (np.asarray(it).astype(u) << u(28)) + (u(stream) << u(24)) + np.asarray(index).astype(u)
        x = u(seed & M64) * u(0xD1342543DE82EF95) + (ctr + u(1)) * u(0x9E3779B97F4A7C15)
        x = x ^ (x >> u(30))
        x = x * u(0xBF58476D1CE4E5B9)
        x = x ^ (x >> u(27))
        x = x * u(0x94D049BB133111EB)
        x = x ^ (x >> u(31))
    return x


def uniforms(seed, its, stream, n):
    """u[i, j] of iterations `its`, one stream, indices 0..n-1: the top 53 bits, [0, 1)."""
    k = mix64(seed, np.asarray(its)[:, None], stream, np.arange(n)[None, :])
    return (k >> np.uint64(11)).astype(np.float64) * (1.0 / 9007199254740992.0)


def test_array_arithmetic_is_the_integer_arithmetic():
    rng = np.random.default_rng(1)
    for seed in (0, 17, 2**63 + 5, M64):
        its, idx = rng.integers(0, 1 << 20, size=20), rng.integers(0, 4096, size=20)
        for stream in range(7):
            got = mix64(seed, its, stream, idx)
            assert [int(g) for g in got] == [mix64_int(seed, int(i), stream, int(j)) for i, j in zip(its, idx)]


@pytest.mark.parametrize('nw', [12, 18, 4096])
def test_counter_draws_is_that_arithmetic_and_a_later_chunk_is_the_streams_later_rows(nw):
    seed, a, ns = 2**63 + 5, 2.0, nw // 2
    whole = counter_draws(seed, a, NDIM, 0, 11, nw)
    later = counter_draws(seed, a, NDIM, 5, 6, nw)
    for w, l in zip(whole, later):
        assert l.shape == (6, 2, ns) and np.array_equal(l, w[5:])
    sidx, cidx, partner, zz, zfac, logu = whole
    keys = mix64(seed, np.arange(11)[:, None], 0, np.arange(nw)[None, :])
    perm = np.argsort(keys, axis=1, kind='stable')
    assert np.array_equal(sidx.reshape(11, nw), perm) and np.array_equal(cidx, sidx[:, ::-1])
    for h in (0, 1):
        uz, up, ua = (uniforms(seed, np.arange(11), k + 3 * h, ns) for k in (1, 2, 3))
        assert np.array_equal(zz[:, h], ((a - 1.0) * uz + 1.0) ** 2 / a)
        assert np.array_equal(partner[:, h], np.minimum((up * ns).astype(np.int32), ns - 1))
        assert np.array_equal(logu[:, h], np.log(ua)) and np.array_equal(zfac[:, h], (NDIM - 1.0) * np.log(zz[:, h]))


@pytest.mark.parametrize('nw', [12, 4096])
def test_the_counter_does_not_alias_across_its_fields(nw):
    """Iterations 0..63, all 7 streams, every index a run of nw walkers uses (nw keys, nw / 2 per half-step stream): the
    counters are pairwise distinct -- no (iteration, stream, index) shares another's -- and so are the 64-bit outputs (the
    mix is a bijection of the counter for a fixed seed, so the second follows from the first).  This is a statement about
    the packing as it is WRITTEN HERE, mix64 above: the library's counter_mix64 is a C function without a Python accessor,
    so nothing in this test reads the kernel's packing.  What ties the two together is counter_draws against this
    arithmetic (the test above) and the device against counter_draws (tests/test_gpu_overlap.py)."""
    seed, its = 2024, np.arange(64)[:, None]
    ctrs, keys = [], []
    for stream in range(7):
        idx = np.arange(nw if stream == 0 else nw // 2)[None, :]
        ctrs.append(((its.astype(np.uint64) << np.uint64(28)) + (np.uint64(stream) << np.uint64(24)) + idx.astype(np.uint64)).ravel())
        keys.append(mix64(seed, its, stream, idx).ravel())
    ctrs, keys = np.concatenate(ctrs), np.concatenate(keys)
    assert len(keys) == 64 * (nw + 6 * (nw // 2))
    assert len(np.unique(ctrs)) == len(ctrs)
    assert len(np.unique(keys)) == len(keys)
    # the widths leave room: the largest index and stream in use, against their fields
    assert nw - 1 < 1 << IDX_BITS and 6 < 1 << STREAM_BITS and DeviceGroupSampler.DEVICE_RNG_MAX_WALKERS - 1 < 1 << IDX_BITS


# The correlation checks: N pairs of uniforms, |r| < 5 / sqrt(N) -- five standard errors of the sample correlation of
# independent uniforms (1 / sqrt(N)).  N = 32 iterations x 4096 u_z (4096 walkers: two half-steps of 2048) = 131072, bound
# 0.0138.  The same bound holds for NumPy's own generator on the same shapes (the control below), so a failure is the
# counter stream's.
N_IT, N_PER_IT = 32, 4096
N = N_IT * N_PER_IT
BOUND = 5.0 / np.sqrt(N)
CORR_SEEDS = (1, 2024, 2**63 + 5)


def u_z(seed, its):
    """The u_z of the iterations `its` of a 4096-walker run: streams 1 and 4, indices 0..2047 -> (len(its), 4096)."""
    return np.concatenate([uniforms(seed, its, 1, N_PER_IT // 2), uniforms(seed, its, 4, N_PER_IT // 2)], axis=1)


def corr(x, y):
    return float(np.corrcoef(x.ravel(), y.ravel())[0, 1])


def test_the_bound_is_one_independent_uniforms_meet():
    for seed in CORR_SEEDS:
        g = np.random.default_rng(seed)
        x, y = g.random((N_IT, N_PER_IT)), g.random((N_IT, N_PER_IT))
        assert x.size == N and abs(corr(x, y)) < BOUND, (seed, corr(x, y), BOUND)
        z = g.random((N_IT + 1, N_PER_IT))
        assert abs(corr(z[:-1], z[1:])) < BOUND


@pytest.mark.parametrize('seed', CORR_SEEDS)
def test_neighbouring_iterations_and_neighbouring_seeds_do_not_correlate(seed):
    u = u_z(seed, np.arange(N_IT + 1))
    assert u[:-1].size == N and 0.0 <= u.min() and u.max() < 1.0
    r_it = corr(u[:-1], u[1:])                       # iteration i against i + 1, index by index
    r_seed = corr(u[:-1], u_z((seed + 1) & M64, np.arange(N_IT)))   # seed s against s + 1, draw by draw
    print('seed {}: r(i, i + 1) = {:+.5f}, r(s, s + 1) = {:+.5f}, bound {:.5f}'.format(seed, r_it, r_seed, BOUND))
    assert abs(r_it) < BOUND, (r_it, BOUND)
    assert abs(r_seed) < BOUND, (r_seed, BOUND)
    # ... and they are uniform: mean 1/2 and variance 1/12 within five standard errors (sqrt(1/12N), sqrt(1/180N))
    assert abs(u[:-1].mean() - 0.5) < 5.0 * np.sqrt(1.0 / (12 * N))
    assert abs(u[:-1].var() - 1.0 / 12) < 5.0 * np.sqrt(1.0 / (180 * N))
