"""CPU: moves and sets of moves on the host samplers (mcmc_spec_amd.moves, sampler.EnsembleSampler, group.GroupSampler;
DESIGN.md section 16): the three forms of ``moves=`` and the refusals; ``moves=None`` and a lone ``StretchMove`` through the
code path the samplers have always had; the host loop against a plain-Python restatement (tests/moves_numpy.py) on a fixed
draw; the counter generator's new streams; stationarity on a Gaussian and the mode weights of a bimodal target; and what
``DeviceEnsembleSampler(moves=...)`` asks of a context (a recording one: no library, no GPU)."""
import numpy as np
import pytest

import common  # noqa: F401
import moves_numpy as mn
from mcmc_spec_amd.group import DeviceGroupSampler, GroupSampler
from mcmc_spec_amd.moves import DEMove, MoveSet, StretchMove, counter_draws_moves, de_pair, parse_moves
from mcmc_spec_amd.sampler import DeviceEnsembleSampler, EnsembleSampler, State, counter_draws
from test_group_rng_abi import StubGroup
from test_sampler_rng_abi import RecordingContext, StubEngine, mix64


def mix():
    return [(StretchMove(), 0.5), (DEMove(), 0.4), (DEMove(gamma0=1.0), 0.1)]


def gauss(x):
    return -0.5 * np.sum(x * x, axis=1)


# ---- 1. the argument -----------------------------------------------------------------------------------------------------
def test_the_three_forms_of_moves_are_accepted():
    one = parse_moves(DEMove())
    assert isinstance(one, MoveSet) and len(one) == 1 and one.weights.tolist() == [1.0]
    equal = parse_moves([StretchMove(), DEMove()])
    assert equal.kinds == [0, 1] and equal.weights.tolist() == [0.5, 0.5]
    weighted = parse_moves([(StretchMove(), 2), (DEMove(), 1.0), (DEMove(gamma0=1.0), 1)])
    assert weighted.weights.tolist() == [0.5, 0.25, 0.25] and weighted.cum[-1] == 1.0
    assert weighted.gamma0(1, 6) == 2.38 / np.sqrt(12.0) and weighted.gamma0(2, 6) == 1.0
    for mv in (DEMove(), [StretchMove(), DEMove()], mix()):
        assert EnsembleSampler(12, 3, gauss, vectorize=True, moves=mv)._moves is not None
        assert GroupSampler([12, 16], 3, None, moves=mv)._moves is not None
        assert DeviceEnsembleSampler(16, 6, StubEngine(), moves=mv)._moves is not None
        assert DeviceGroupSampler([16], 6, StubGroup(1), moves=mv)._moves is not None
    from mcmc_spec_amd import mft6
    import inspect
    assert 'moves' in inspect.signature(mft6.device_sampler).parameters


@pytest.mark.parametrize('bad', [[StretchMove()] * 5, 'stretch', object(), [DEMove(), 3.0], [(DEMove(), 0.0)], [(DEMove(), -1.0)],
                                 [(DEMove(), float('nan'))], [(DEMove(), float('inf'))], [], [(DEMove(), 1.0, 2.0)]],
                         ids=['five', 'str', 'object', 'number', 'w=0', 'w<0', 'w=nan', 'w=inf', 'empty', 'triple'])
def test_refusals_raise_value_error(bad):
    with pytest.raises(ValueError):
        EnsembleSampler(12, 3, gauss, vectorize=True, moves=bad)
    with pytest.raises(ValueError):
        DeviceEnsembleSampler(16, 6, StubEngine(), moves=bad)


def test_a_and_moves_exclude_each_other_and_the_sharded_run_is_stretch_only():
    for make in (lambda **kw: EnsembleSampler(12, 3, gauss, vectorize=True, **kw), lambda **kw: DeviceEnsembleSampler(16, 6, StubEngine(), **kw),
                 lambda **kw: GroupSampler([12], 3, None, **kw), lambda **kw: DeviceGroupSampler([16], 6, StubGroup(1), **kw)):
        with pytest.raises(ValueError, match='exclude'):
            make(a=2.0, moves=DEMove())
        with pytest.raises(ValueError, match='exclude'):
            make(a=3.0, moves=StretchMove(3.0))
    assert EnsembleSampler(12, 3, gauss, a=3.0).a == 3.0 and EnsembleSampler(12, 3, gauss).a == 2.0
    assert EnsembleSampler(12, 3, gauss, moves=StretchMove(3.0)).a == 3.0
    with pytest.raises(ValueError):
        StretchMove(1.0)
    with pytest.raises(ValueError):
        DEMove(gamma0=0.0)
    with pytest.raises(ValueError, match='stretch only'):
        DeviceEnsembleSampler(16, 6, StubEngine(), moves=mix(), shard=(0, 2), seed=1)
    assert DeviceEnsembleSampler(16, 6, StubEngine(), moves=StretchMove(), shard=(0, 2), seed=1)._moves is None
    assert DeviceEnsembleSampler(16, 6, StubEngine(), moves=mix(), shard=(0, 1))._moves is not None
    with pytest.raises(ValueError, match='4 walkers'):
        EnsembleSampler(2, 1, gauss, moves=DEMove())


# ---- 2. today's path -------------------------------------------------------------------------------------------------------
def test_none_and_a_lone_stretch_move_walk_todays_chain():
    p0 = np.random.default_rng(0).normal(size=(16, 3))
    today = EnsembleSampler(16, 3, gauss, vectorize=True, seed=9)
    today.run_mcmc(p0, 60)
    for kw in (dict(moves=None), dict(moves=StretchMove(2.0)), dict(moves=[StretchMove(2.0)]), dict(moves=[(StretchMove(2.0), 3.0)])):
        s = EnsembleSampler(16, 3, gauss, vectorize=True, seed=9, **kw)
        assert s._moves is None and len(s._draw_steps(1)) == 6      # (the stretch move's own layout: its own path)
        s = EnsembleSampler(16, 3, gauss, vectorize=True, seed=9, **kw)
        s.run_mcmc(p0, 60)
        assert np.array_equal(s.get_chain(), today.get_chain()) and np.array_equal(s.get_log_prob(), today.get_log_prob())
        assert np.array_equal(s.acceptance_fraction, today.acceptance_fraction)
    # ... and forced through the general path: the general layout, the same numbers, the same chain
    g = EnsembleSampler(16, 3, gauss, vectorize=True, seed=9, moves=StretchMove(2.0), _general=True)
    t = EnsembleSampler(16, 3, gauss, vectorize=True, seed=9)
    dg, dt = g._draw_steps(3), t._draw_steps(3)
    assert len(dg) == 8 and np.array_equal(dg[2], [0, 0, 0])
    for i, j in ((0, 0), (1, 1), (3, 2), (4, 2), (5, 3), (6, 4), (7, 5)):
        assert np.array_equal(dg[i], dt[j]), (i, j)
    g = EnsembleSampler(16, 3, gauss, vectorize=True, seed=9, moves=StretchMove(2.0), _general=True)
    g.run_mcmc(p0, 60)
    assert np.array_equal(g.get_chain(), today.get_chain()) and np.array_equal(g.acceptance_fraction, today.acceptance_fraction)
    a25 = EnsembleSampler(16, 3, gauss, vectorize=True, seed=9, a=2.5)
    m25 = EnsembleSampler(16, 3, gauss, vectorize=True, seed=9, moves=StretchMove(2.5))
    a25.run_mcmc(p0, 20), m25.run_mcmc(p0, 20)
    assert np.array_equal(a25.get_chain(), m25.get_chain()) and not np.array_equal(a25.get_chain(), today.get_chain()[:20])


# ---- 3. the host loop on a fixed draw, against the plain-Python restatement ---------------------------------------------
def _fixed_draw(m, nw, ndim, seed):
    """m iterations in the general layout from a generator of the test's own: kinds alternate, DE pairs distinct."""
    r = np.random.default_rng(seed)
    ns = nw // 2
    perm = np.stack([r.permutation(nw) for _ in range(m)]).astype(np.int32).reshape(m, 2, ns)
    kind = (np.arange(m) % 3 != 0).astype(np.int32)
    p1 = r.integers(0, ns, size=(m, 2, ns)).astype(np.int32)
    p2 = ((p1 + r.integers(1, ns, size=(m, 2, ns))) % ns).astype(np.int32)
    g = np.where(kind[:, None, None] == 0, r.uniform(0.5, 2.0, size=(m, 2, ns)), 0.7 * (1.0 + 1e-2 * r.normal(size=(m, 2, ns))))
    p2[kind == 0] = p1[kind == 0]
    fac = np.where(kind[:, None, None] == 0, (ndim - 1.0) * np.log(g), 0.0)
    logu = np.log(r.random((m, 2, ns)))
    return perm, np.ascontiguousarray(perm[:, ::-1]), kind, p1, p2, g, fac, logu


def test_the_host_loop_is_the_plain_python_restatement_bit_for_bit():
    m, nw, ndim = 30, 14, 4
    d = _fixed_draw(m, nw, ndim, 3)
    assert np.all(d[3][d[2] == 1] != d[4][d[2] == 1])

    def lp(x):   # a box (rejections by -inf, and -inf - -inf = nan never accepts) around a tilted Gaussian
        out = -0.5 * np.sum((x - 0.3) ** 2 * np.arange(1, ndim + 1), axis=1)
        return np.where(np.any(np.abs(x) > 2.5, axis=1), -np.inf, out)

    p0 = np.random.default_rng(4).normal(size=(nw, ndim))
    p0[0] = 3.0   # one walker starts outside the box: ln p = -inf
    s = EnsembleSampler(nw, ndim, lp, vectorize=True, moves=mix(), draws=lambda i, k: tuple(a[i:i + k] for a in d))
    s.run_mcmc(p0, m)
    coords, logp = p0.copy(), lp(p0)
    nacc = np.zeros(nw)
    for i in range(m):
        nacc += mn.iterate(coords, logp, lp, *[a[i] for a in d])
        assert np.array_equal(s.get_chain()[i], coords) and np.array_equal(s.get_log_prob()[i], logp), i
    assert np.array_equal(s.acceptance_fraction, nacc / m) and 0.1 < nacc.mean() / m < 0.9
    # the group sampler runs the same function per target
    gs = GroupSampler([nw, nw], ndim, lambda cs: [lp(c) for c in cs], moves=mix(),
                      draws=[lambda i, k: tuple(a[i:i + k] for a in d)] * 2)
    gs.run_mcmc([p0, p0], m)
    assert np.array_equal(gs.get_chain(0), s.get_chain()) and np.array_equal(gs.get_chain(1), s.get_chain())


# ---- 4. the counter generator's new streams --------------------------------------------------------------------------------
def test_streams_0_to_6_do_not_change_with_a_set():
    seed, nw, ndim = 2**63 + 5, 18, 6
    plain = counter_draws(seed, 2.0, ndim, 3, 9, nw)
    got = counter_draws_moves(seed, mix(), ndim, 3, 9, nw)
    assert len(got) == 8 and got[2].shape == (9,) and got[2].dtype == np.int32 and all(a.shape == (9, 2, 9) for a in got[:2] + got[3:])
    st = got[2] == 0
    assert st.any() and (~st).any()
    assert np.array_equal(got[0], plain[0]) and np.array_equal(got[1], plain[1]) and np.array_equal(got[7], plain[5])
    for i, j in ((3, 2), (4, 2), (5, 3), (6, 4)):
        assert np.array_equal(got[i][st], plain[j][st]), (i, j)
    assert np.all(got[6][~st] == 0.0)
    # a pure-stretch set is the stretch-only generator, and a later chunk is the stream's later rows
    pure = counter_draws_moves(seed, StretchMove(2.0), ndim, 3, 9, nw)
    assert np.all(pure[2] == 0) and all(np.array_equal(pure[i], plain[j]) for i, j in ((3, 2), (4, 2), (5, 3), (6, 4), (7, 5)))
    whole = counter_draws_moves(seed, mix(), ndim, 0, 12, nw)
    assert all(np.array_equal(a[3:], b) for a, b in zip(whole, got))


def test_the_new_fields_are_the_packing_in_python_integers():
    seed, nw, ndim, ns = 2024, 12, 6, 6
    got = counter_draws_moves(seed, mix(), ndim, 5, 8, nw)
    cum = np.cumsum([0.5, 0.4, 0.1])
    kinds, g0 = [0, 1, 1], [None, 2.38 / np.sqrt(12.0), 1.0]
    for i in range(8):
        it = 5 + i
        u = mn.uniform_int(seed, it, 7, 0)
        which = next((k for k in range(3) if u < cum[k]), 2)
        assert got[2][i] == kinds[which]
        if kinds[which] == 0:
            continue
        for h in (0, 1):
            for j in range(ns):
                j1, j2 = mn.de_pair_int(mn.uniform_int(seed, it, 8 + 3 * h, j), ns)
                assert (got[3][i, h, j], got[4][i, h, j]) == (j1, j2) and j1 != j2
                u1, u2 = mn.uniform_int(seed, it, 9 + 3 * h, j), mn.uniform_int(seed, it, 10 + 3 * h, j)
                n = np.sqrt(-2.0 * np.log(1.0 - u1)) * np.cos(6.283185307179586 * u2)
                assert np.isclose(got[5][i, h, j], g0[which] * (1.0 + 1e-5 * n), rtol=4e-16, atol=0)   # (array log / cos against the scalar ones)


def test_no_two_of_the_fourteen_fields_alias():
    """Streams 0..13 (the split's keys; u_z, u_p, u_a and the DE pair and the two Box-Muller uniforms of either half-step; the
    move's choice) over 64 iterations: pairwise distinct counters and outputs, every stream inside the field's 4 bits."""
    seed, nw, its = 2024, 4096, np.arange(64)[:, None]
    sizes = {0: nw, 7: 1}
    ctrs, keys = [], []
    for stream in range(14):
        assert stream < 1 << 4
        idx = np.arange(sizes.get(stream, nw // 2))[None, :]
        ctrs.append(((its.astype(np.uint64) << np.uint64(28)) + (np.uint64(stream) << np.uint64(24)) + idx.astype(np.uint64)).ravel())
        keys.append(mix64(seed, its, stream, idx).ravel())
    ctrs, keys = np.concatenate(ctrs), np.concatenate(keys)
    assert len(keys) == 64 * (nw + 1 + 12 * (nw // 2))
    assert len(np.unique(ctrs)) == len(ctrs) and len(np.unique(keys)) == len(keys)
    assert int(mix64(seed, np.array([3]), 9, np.array([5]))[0]) == mn.mix64_int(seed, 3, 9, 5)


def test_the_de_pair_is_never_diagonal_and_reaches_every_ordered_pair():
    for nc in (2, 3, 5, 9, 257, 2048):
        u = np.concatenate([np.random.default_rng(nc).random(20000), [0.0, np.nextafter(1.0, 0.0)]])
        j1, j2 = de_pair(u, nc)
        assert np.all(j1 != j2) and j1.min() >= 0 and j2.min() >= 0 and j1.max() < nc and j2.max() < nc
        assert all((int(a), int(b)) == mn.de_pair_int(float(x), nc) for x, a, b in zip(u[:50], j1, j2))
    npairs = 6
    j1, j2 = de_pair((np.arange(npairs) + 0.5) / npairs, 3)
    assert sorted(zip(j1.tolist(), j2.tolist())) == [(a, b) for a in range(3) for b in range(3) if a != b]
    # ... and through the generator: 3 walkers per half, every ordered pair occurs
    got = counter_draws_moves(11, DEMove(), 3, 0, 40, 6)
    assert set(zip(got[3].ravel().tolist(), got[4].ravel().tolist())) == {(a, b) for a in range(3) for b in range(3) if a != b}


# ---- 5. what the moves sample ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', ['DE', 'DE + jump', 'mixture'])
def test_stationarity_on_a_unit_gaussian(name):
    """5-D unit Gaussian, 40 walkers started at 3 +- 0.1, 4,000 iterations, the first 1,000 discarded: every |mean| <= 0.1
    and every variance in [0.9, 1.1] (the specification's restatement gave <= 0.044 and [0.96, 1.03] over 8 seeds)."""
    mv = {'DE': DEMove(), 'DE + jump': [(DEMove(), 0.9), (DEMove(gamma0=1.0), 0.1)], 'mixture': mix()}[name]
    s = EnsembleSampler(40, 5, gauss, vectorize=True, seed=3, moves=mv)
    s.run_mcmc(3.0 + 0.1 * np.random.default_rng(1).normal(size=(40, 5)), 4000)
    c = s.get_chain(discard=1000, flat=True)
    mean, var = c.mean(axis=0), c.var(axis=0)
    print(name, 'max |mean|', np.abs(mean).max(), 'variances', var.min(), var.max(), 'acceptance', s.acceptance_fraction.mean())
    assert np.all(np.abs(mean) <= 0.1) and np.all(var >= 0.9) and np.all(var <= 1.1)


def bimodal(x):
    """Two unit Gaussians in 6-D, 10 sigma apart along x0 (at -5 and +5), weights 0.8 / 0.2."""
    r2 = np.sum(x[:, 1:] ** 2, axis=1)
    return np.logaddexp(np.log(0.8) - 0.5 * ((x[:, 0] + 5.0) ** 2 + r2), np.log(0.2) - 0.5 * ((x[:, 0] - 5.0) ** 2 + r2))


def _heavy_fraction(moves):
    p0 = np.random.default_rng(2).normal(size=(50, 6))
    p0[:25, 0] -= 5.0
    p0[25:, 0] += 5.0
    s = EnsembleSampler(50, 6, bimodal, vectorize=True, seed=5, moves=moves)
    s.run_mcmc(p0, 3000)
    return float(np.mean(s.get_chain(discard=1500, flat=True)[:, 0] < 0.0))


def test_mode_weights_of_a_bimodal_target():
    """50 walkers started 25 / 25, 3,000 iterations, the second half counted: the stretch move alone leaves the x0 < 0
    fraction <= 0.70 (walkers do not change mode: 0.50-0.66 over 25 seeds of the specification's restatement), the
    three-move mixture gives 0.73-0.87 (0.76-0.83 there) for the true 0.8."""
    stretch, mixture = _heavy_fraction(None), _heavy_fraction(mix())
    print('x0 < 0 fraction: stretch', stretch, ' mixture', mixture)
    assert stretch <= 0.70
    assert 0.73 <= mixture <= 0.87


# ---- 6. what DeviceEnsembleSampler(moves=...) asks of a context -------------------------------------------------------------
class MovesContext(RecordingContext):
    def sampler_enqueue_moves_drawn(self, slot, nsteps, seed, moves, first_iter):
        assert slot not in self.pending, 'slot not collected yet'
        self.calls.append(('moves_drawn', slot, nsteps, seed, moves, first_iter))
        self.pending[slot] = nsteps
        return nsteps

    def sampler_enqueue_moves(self, slot, *arrays):
        assert slot not in self.pending, 'slot not collected yet'
        self.calls.append(('moves', slot, arrays))
        self.pending[slot] = len(arrays[2])
        return len(arrays[2])

    def sampler_enqueue_drawn(self, *a):
        raise AssertionError('a set of moves goes through msx_sampler_enqueue_moves_drawn')


class MovesEngine(StubEngine):
    def __init__(self, nw=16, ndim=6):
        self.ctx = MovesContext(nw, ndim)


def test_the_device_sampler_queues_moves_chunks_at_the_absolute_iteration():
    """Runs of 5 and 6 iterations at chunk = 4: chunks of 4 + 1 and 4 + 2, first iterations 0, 4 | 5, 9; plain launches."""
    eng = MovesEngine()
    s = DeviceEnsembleSampler(16, 6, eng, seed=11, chunk=4, rng='device', moves=mix())
    st = s.run_mcmc(State(np.random.default_rng(0).normal(size=(16, 6)), np.zeros(16)), 5)
    assert s._drawn == 5 and s.overlapped is False
    s.reset()
    assert s._drawn == 5 and s.iteration == 0
    s.run_mcmc(st, 6)
    assert s._drawn == 11 and s.get_chain().shape == (6, 16, 6)
    calls = eng.ctx.calls
    drawn = [c for c in calls if c[0] == 'moves_drawn']
    assert [c[5] for c in drawn] == [0, 4, 5, 9] and [c[2] for c in drawn] == [4, 1, 4, 2]
    assert all(c[3] == 11 and c[4] is s._moves and len(c[4]) == 3 for c in drawn)
    assert [c for c in calls if c[0] == 'policy'] == [('policy', 0)] * 2          # plain launches, asked for before begin
    assert [c[0] for c in calls].index('policy') < [c[0] for c in calls].index('begin')
    assert not [c for c in calls if c[0] in ('drawn', 'shard')]
    # world 1 is one GPU: taken, and nothing is sharded; world > 1 raises before anything is queued
    eng1 = MovesEngine()
    DeviceEnsembleSampler(16, 6, eng1, seed=11, chunk=4, rng='device', moves=mix(), shard=(0, 1)).run_mcmc(st, 2)
    assert not [c for c in eng1.ctx.calls if c[0] == 'shard'] and [c[5] for c in eng1.ctx.calls if c[0] == 'moves_drawn'] == [0]
    with pytest.raises(ValueError, match='stretch only'):
        DeviceEnsembleSampler(16, 6, MovesEngine(), seed=11, rng='device', moves=mix(), shard=(1, 2))


def test_the_host_drawn_device_sampler_uploads_the_general_layout():
    eng = MovesEngine()
    s = DeviceEnsembleSampler(16, 6, eng, seed=11, chunk=4, moves=mix())
    s.run_mcmc(State(np.zeros((16, 6)), np.zeros(16)), 6)
    chunks = [c[2] for c in eng.ctx.calls if c[0] == 'moves']
    assert [len(a[2]) for a in chunks] == [4, 2] and all(len(a) == 8 for a in chunks)
    twin = EnsembleSampler(16, 6, gauss, vectorize=True, seed=11, moves=mix())
    want = twin._draw_steps(6)
    for i in range(8):
        assert np.array_equal(np.concatenate([a[i] for a in chunks]), want[i]), i
    assert s.overlapped is False and ('policy', 0) in eng.ctx.calls
