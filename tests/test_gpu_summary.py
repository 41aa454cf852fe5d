"""GPU: order statistics and binned marginals of chains held on the device (include/msx.h, msx_series_order_stats /
_hist / _hist2d; mcmc_spec_amd.summary; the samplers' get_summary).  Everything is selected elements
and integer counts, so every comparison with the NumPy restatements (tests/summary_numpy.py) is exact."""
import numpy as np
import pytest

from common import golden_case
from summary_numpy import (chain_like, flat_members, loop_counts, numpy_counts, numpy_counts2d, order_stats,
                           reference_counts)
from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu

COUNTS = (2, 6, 4)
SIZES = (1, 2, 63, 64, 65, 257)          # n': one short of, at and one past a wave; a few waves
BIG = 4099                                # ... and one past a tile of 4,096 rows
SELECTIONS = ((0, 1), (5, 1), (0, 3), (7, 4))


def _eng():
    import common
    if 'summary_engA' not in common._cache:
        common._cache['summary_engA'] = make_engine(golden_case('A'))
    return common._cache['summary_engA']


def _series(x, counts=None, **kw):
    from mcmc_spec_amd import _lib
    ser = _lib.Series(_eng().ctx, x.shape[1], x.shape[2], counts, **kw)
    ser.append(x)
    return ser


def test_the_restatement_is_the_references_loop():
    """Pins tests/summary_numpy.py to the reference's statements (mft6.py:2046-2049) before anything is compared with it."""
    rng = np.random.default_rng(1)
    x = rng.normal(size=200)
    edges = np.linspace(x.min(), x.max(), 75)
    assert np.array_equal(reference_counts(x, edges), loop_counts(x, edges))


def _values(kind, n, nw, ndim):
    rng = np.random.default_rng(len(kind) * 7 + 1)
    if kind == 'binades':      # normal draws spanning sign and ten binades
        return rng.normal(size=(n, nw, ndim)) * 2.0 ** rng.integers(-5, 5, size=(n, nw, ndim))
    if kind == 'three':        # three distinct values
        return np.array([-1.5, 0.25, 3e7])[rng.integers(0, 3, size=(n, nw, ndim))]
    if kind == 'equal':
        return np.full((n, nw, ndim), 0.1)
    if kind == 'chain':        # each row copied from the previous one with probability 0.7
        return chain_like(n, nw, ndim, 5, repeat=0.7, scale=np.array([30.0, 0.02, 2e-5]))
    x = rng.normal(size=(n, nw, ndim))   # 'nonfinite': +-inf and NaN among them (NaN of either sign bit)
    x[rng.random((n, nw, ndim)) < 0.02] = np.inf
    x[rng.random((n, nw, ndim)) < 0.02] = -np.inf
    x[rng.random((n, nw, ndim)) < 0.02] = np.nan
    x[3, 1, 0], x[0, 0, 1] = -np.nan, np.copysign(np.nan, -1.0)
    return x


@pytest.mark.parametrize('kind', ['binades', 'three', 'equal', 'chain', 'nonfinite'])
def test_order_statistics_at_every_rank(kind):
    """k = 3 members of (2, 6, 4) walkers, ndim 3: every rank 0 .. N_m - 1 in one call at the small sizes, the ends, the
    middle and the 16 / 50 / 84 ranks at 4,099 rows, for four (discard, thin)."""
    nw, ndim = sum(COUNTS), 3
    x = _values(kind, 7 + 4 * (BIG - 1) + 1, nw, ndim)
    ser = _series(x, COUNTS)
    w = np.array(COUNTS)
    for discard, thin in SELECTIONS:
        for npr in SIZES + (BIG,):
            n = discard + thin * (npr - 1) + 1
            big = npr * w
            if npr < BIG:
                ranks = np.minimum(np.arange(big.max())[None, :], big[:, None] - 1)
            else:
                h = (big[:, None] - 1) * np.array([0.16, 0.5, 0.84])[None, :]
                lo = np.floor(h).astype(np.int64)
                ranks = np.concatenate([np.stack([0 * big, 0 * big + 1, big // 2 - 1, big // 2, big - 2, big - 1], axis=1), lo,
                                        np.minimum(lo + 1, big[:, None] - 1)], axis=1)
            got, count = ser.order_stats(n, discard, thin, [0, 1, 2], ranks)
            assert np.array_equal(count, big)
            flats = flat_members(x, n, discard, thin, COUNTS)
            for m in range(3):
                assert flats[m].shape[0] == big[m]
                for j in range(ndim):
                    want = order_stats(flats[m][:, j], ranks[m])
                    assert np.array_equal(got[m, j], want, equal_nan=True), (kind, discard, thin, npr, m, j)
    ser.close()


def test_rows_beyond_n_and_growth():
    from mcmc_spec_amd import _lib
    rng = np.random.default_rng(8)
    x = rng.normal(size=(300, 5, 2))
    x[200:] = 1e300                                   # a sentinel past n = 200: must not show in max
    ser = _series(x)
    got, count = ser.order_stats(200, 0, 1, [0, 1], [[0, 500, 999]])
    flat = flat_members(x, 200)[0]
    assert count[0] == 1000 and got.max() < 1e300
    assert np.array_equal(got[0], np.array([order_stats(flat[:, j], [0, 500, 999]) for j in range(2)]))
    edges = np.tile(np.linspace(-3.0, 3.0, 20), (1, 2, 1))
    assert np.array_equal(ser.hist(200, 0, 1, [0, 1], edges)[0, 1], numpy_counts(flat[:, 1], edges[0, 1]))
    ser.close()
    # two reallocations (cap_hint 16, pieces of 10 and 50 rows) against one allocation
    a = _lib.Series(_eng().ctx, 5, 2, cap_hint=16)
    a.append(x[:10])
    a.append(x[10:60])
    b = _lib.Series(_eng().ctx, 5, 2, cap_hint=64)
    b.append(x[:60])
    ranks = [np.arange(145)]                           # rows 3, 5 .. 59: 29 rows x 5 walkers
    ga, gb = a.order_stats(60, 3, 2, [1, 0], ranks), b.order_stats(60, 3, 2, [1, 0], ranks)
    assert np.array_equal(ga[0], gb[0]) and ga[1][0] == gb[1][0] == 145
    flat = flat_members(x, 60, 3, 2)[0]
    assert np.array_equal(ga[0][0, 0], np.sort(flat[:, 1])) and np.array_equal(ga[0][0, 1], np.sort(flat[:, 0]))
    assert np.array_equal(a.hist(60, 3, 2, [0, 1], edges), b.hist(60, 3, 2, [0, 1], edges))
    a.close()
    b.close()


def test_ratio_column_is_the_correctly_rounded_quotient():
    """MSX_COL_RATIO(1, 0) against np.sort(x1 / x0): random 53-bit mantissas, denominators of both signs -- the quotient's
    last bit then depends on correct rounding."""
    from mcmc_spec_amd import _lib
    rng = np.random.default_rng(19)
    shape = (301, 6, 2)
    x = rng.integers(2 ** 52, 2 ** 53, size=shape).astype(np.float64) * 2.0 ** rng.integers(-60, -44, size=shape)
    x *= rng.choice([-1.0, 1.0], size=shape)
    ser = _series(x, (4, 2))
    n, discard, thin = 301, 2, 3
    flats = flat_members(x, n, discard, thin, (4, 2))
    big = np.array([f.shape[0] for f in flats])
    ranks = np.minimum(np.arange(big.max())[None, :], big[:, None] - 1)
    got, _ = ser.order_stats(n, discard, thin, [_lib.col_ratio(1, 0), 1, _lib.col_ratio(0, 1)], ranks)
    for m, f in enumerate(flats):
        assert np.array_equal(got[m, 0], np.sort(f[:, 1] / f[:, 0])[ranks[m]]), m
        assert np.array_equal(got[m, 1], np.sort(f[:, 1])[ranks[m]]), m
        assert np.array_equal(got[m, 2], np.sort(f[:, 0] / f[:, 1])[ranks[m]]), m
    num, den = np.concatenate([f[:, 1] for f in flats]), np.concatenate([f[:, 0] for f in flats])
    assert np.sum(num / den != num * (1.0 / den)) > 50      # (a quotient by reciprocal would miss the last bit of these)
    edges = np.stack([np.linspace(np.min(f[:, 1] / f[:, 0]), np.max(f[:, 1] / f[:, 0]), 75) for f in flats])[:, None, :]
    counts = ser.hist(n, discard, thin, [_lib.col_ratio(1, 0)], edges, closed_last=False)
    for m, f in enumerate(flats):
        assert np.array_equal(counts[m, 0], reference_counts(f[:, 1] / f[:, 0], edges[m, 0])[:-1]), m
    ser.close()


def _edge_data(edges, seed):
    rng = np.random.default_rng(seed)
    a, b = edges[0], edges[-1]
    inside = a + (b - a) * rng.random(500)
    outside = np.concatenate([a - (b - a) * (0.01 + rng.random(10)), b + (b - a) * (0.01 + rng.random(10))])
    x = np.concatenate([edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf), inside, outside, [np.nan, b, b]])
    return rng.permutation(x)


@pytest.mark.parametrize('nedges', [2, 3, 75, 4097])
def test_histogram_edge_rule(nedges):
    """Every np.linspace edge, its two neighbours, values inside and outside, NaN: both conventions for the last edge."""
    edges = np.linspace(-1.7, 2.9, nedges)
    x = _edge_data(edges, nedges)
    nw = 3
    x = np.concatenate([x, np.full(-len(x) % nw, 1e9)])      # (padding outside the edges)
    ser = _series(x.reshape(-1, nw, 1))
    n = len(x) // nw
    for closed in (False, True):
        got = ser.hist(n, 0, 1, [0], edges[None, None, :], closed_last=closed)
        assert got.shape == (1, 1, nedges - 1) and got.dtype == np.int64
        want = numpy_counts(x, edges) if closed else reference_counts(x, edges)[:-1]
        assert np.array_equal(got[0, 0], want), closed
        inside = (x >= edges[0]) & ((x <= edges[-1]) if closed else (x < edges[-1]))
        assert got.sum() == inside.sum()
    on_last = int(np.sum(x == edges[-1]))
    assert on_last == 3
    assert (ser.hist(n, 0, 1, [0], edges[None, None, :], closed_last=True).sum()
            - ser.hist(n, 0, 1, [0], edges[None, None, :], closed_last=False).sum()) == on_last
    ser.close()


def test_histogram_of_two_members_with_their_own_edges():
    x = chain_like(130, 5, 2, 23, repeat=0.5)
    counts = (2, 3)
    ser = _series(x, counts)
    flats = flat_members(x, 130, 4, 3, counts)
    edges = np.empty((2, 2, 75))
    for m in range(2):
        for j in range(2):
            edges[m, j] = np.linspace(flats[m][:, j].min() - 0.1 * m, flats[m][:, j].max() + 0.3 * j, 75)
    for closed in (False, True):
        got = ser.hist(130, 4, 3, [0, 1], edges, closed_last=closed)
        for m in range(2):
            for j in range(2):
                want = numpy_counts(flats[m][:, j], edges[m, j]) if closed else reference_counts(flats[m][:, j], edges[m, j])[:-1]
                assert np.array_equal(got[m, j], want), (closed, m, j)
    ser.close()


@pytest.mark.parametrize('bins', [(1, 1), (3, 7), (50, 50), (128, 128)])
def test_histogram_2d(bins):
    """Three columns, all pairs, two members; rows spanning more than one tile of 16,384; np.histogram2d's edge rule."""
    counts = (1, 2)
    x = chain_like(16391, 3, 3, 29, repeat=0.6)
    ser = _series(x, counts)
    n, discard, thin = 16391, 0, 1
    flats = flat_members(x, n, discard, thin, counts)
    pairs = [(0, 1), (0, 2), (2, 1)]
    ex = np.empty((2, 3, bins[0] + 1))
    ey = np.empty((2, 3, bins[1] + 1))
    for m in range(2):
        for p, (cx, cy) in enumerate(pairs):
            ex[m, p] = np.linspace(flats[m][:, cx].min(), flats[m][:, cx].max(), bins[0] + 1)
            ey[m, p] = np.linspace(flats[m][:, cy].min(), flats[m][:, cy].max() - 0.5 * p, bins[1] + 1)   # (values above the last edge)
    got = ser.hist2d(n, discard, thin, pairs, ex, ey)
    assert got.shape == (2, 3) + bins and got.dtype == np.int64
    for m in range(2):
        for p, (cx, cy) in enumerate(pairs):
            assert np.array_equal(got[m, p], numpy_counts2d(flats[m][:, cx], flats[m][:, cy], ex[m, p], ey[m, p])), (m, p)
    if bins == (128, 128):
        with pytest.raises(ValueError):
            ser.hist2d(n, discard, thin, pairs, np.linspace(0, 1, 130) * np.ones((2, 3, 1)), ey)
        assert np.array_equal(ser.hist2d(n, discard, thin, pairs, ex, ey), got)
    ser.close()


def test_python_layer_on_an_uploaded_chain():
    from mcmc_spec_amd import summary
    counts = (3, 5)
    x = chain_like(211, 8, 6, 31, repeat=0.7, scale=np.array([30.0, 30.0, 0.02, 0.02, 0.02, 2e-5])) + np.array([3500.0, 3300.0, 0.3, 1.0, 0.8, 1e-3])
    ctx = _eng().ctx
    q = [0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0]
    discard, thin = 11, 2
    flats = flat_members(x, 211, discard, thin, counts)
    ratio = summary.col_ratio(4, 3)
    mcols = [0, 1, 3, 4, ratio]                       # T1, T2, R1, R2 and R2 / R1 (mft6.py:2019-2022)
    out = summary.summarize(x, ctx, counts, q=q, discard=discard, thin=thin, marginal={'cols': mcols},
                            corner={'cols': [0, 1, 2, 3, 4, 5]})
    with summary.uploaded(x, ctx, counts) as (ser, n):
        assert n == 211
        assert np.array_equal(summary.quantiles(ser, n, q, discard=discard, thin=thin), out['quantiles'])
        assert np.array_equal(summary.medians(ser, n, discard=discard, thin=thin), out['median'])
        e_np, c_np = summary.marginals(ser, n, mcols, nbins=75, rule='numpy', discard=discard, thin=thin)
    edges, mcounts = out['marginals']
    cedges, c1, pairs, c2 = out['corner']
    assert mcounts.shape == (2, 5, 75) and edges.shape == (2, 5, 75) and c_np.shape == (2, 5, 75) and e_np.shape == (2, 5, 76)
    assert len(pairs) == 15 and c2.shape == (2, 15, 50, 50) and c1.shape == (2, 6, 50)
    for m, f in enumerate(flats):
        assert out['count'][m] == f.shape[0]
        assert np.array_equal(out['quantiles'][m], np.quantile(f, q, axis=0).T)
        assert np.array_equal(out['quantiles'][m][:, 2:5], np.percentile(f, [16, 50, 84], axis=0).T)
        assert np.array_equal(out['median'][m], np.median(f, axis=0))
        assert np.array_equal(out['min'][m], f.min(axis=0)) and np.array_equal(out['max'][m], f.max(axis=0))
        for j, c in enumerate(mcols):
            v = f[:, 4] / f[:, 3] if c == ratio else f[:, c]
            e = np.linspace(min(v), max(v), 75)
            assert np.array_equal(edges[m, j], e)
            assert np.array_equal(mcounts[m, j], reference_counts(v, e)) and mcounts[m, j, -1] == 0
            h, he = np.histogram(v, bins=75)
            assert np.array_equal(e_np[m, j], he) and np.array_equal(c_np[m, j], h)
        for j in range(6):
            h, he = np.histogram(f[:, j], bins=50)
            assert np.array_equal(cedges[m, j], he) and np.array_equal(c1[m, j], h)
        for p, (i, j) in enumerate(pairs):
            assert i > j
            assert np.array_equal(c2[m, p], numpy_counts2d(f[:, j], f[:, i], cedges[m, j], cedges[m, i]))


def _p0(nw, seed=3):
    from mcmc_spec_amd import synth
    c = golden_case('A')
    return synth.draw_walkers(nw, seed=seed, tmin=c.tmin, tmax=c.tmax)


def _host_summary(flat, q=(0.16, 0.5, 0.84)):
    return {'count': flat.shape[0], 'min': flat.min(axis=0), 'max': flat.max(axis=0), 'median': np.median(flat, axis=0),
            'quantiles': np.quantile(flat, q, axis=0).T}


def _same(got, want):
    assert sorted(got) == sorted(want)
    for name in want:
        assert np.array_equal(got[name], want[name]), name


def test_end_to_end_on_a_resident_chain():
    """16 walkers, 60 iterations in chunks of 7 (unequal chunks fill the series); a consumer that breaks mid-chunk and runs
    on (DESIGN.md section 12, rows queued but not consumed); autocorr='host' takes the upload path to the same numbers."""
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    eng = _eng()
    out = {}
    for mode in ('device', 'host'):
        s = DeviceEnsembleSampler(16, 6, eng, seed=5, chunk=7, autocorr=mode)
        st = s.run_mcmc(_p0(16), 60)
        got = s.get_summary(discard=10, thin=2)
        flat = s.get_chain(discard=10, thin=2, flat=True)
        assert flat.shape == (25 * 16, 6)
        _same(got, _host_summary(flat))
        for i, st in enumerate(s.sample(st, iterations=30)):      # breaks mid-chunk: the series holds rows nobody consumed
            if i == 9:
                break
        if mode == 'device':
            assert s._series.rows > len(s._chain) == 70
        _same(s.get_summary(discard=10, thin=2), _host_summary(s.get_chain(discard=10, thin=2, flat=True)))
        s.run_mcmc(st, 15)                                         # ... and runs on: they are overwritten
        assert len(s._chain) == 85
        got = s.get_summary(q=(0.025, 0.5, 0.975), discard=3, thin=4, cols=[4, 0])
        flat = s.get_chain(discard=3, thin=4, flat=True)[:, [4, 0]]
        _same(got, _host_summary(flat, (0.025, 0.5, 0.975)))
        out[mode] = (s.get_summary(), s.get_chain())
    assert np.array_equal(out['device'][1], out['host'][1])
    _same(out['device'][0], out['host'][0])


def test_group_summary_is_each_targets_host_computation():
    from mcmc_spec_amd import synth
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    from test_gpu_target_group import koi_engines
    members = koi_engines()[2][:3]
    c = golden_case('A')
    counts = [12, 16, 12]
    p0s = [synth.draw_walkers(counts[k], seed=70 + k, tmin=c.tmin, tmax=c.tmax) for k in range(3)]
    grp = TargetGroup(members)
    out = {}
    for mode in ('device', 'host'):
        dev = DeviceGroupSampler(counts, 6, grp, seeds=[40, 41, 42], chunk=16, autocorr=mode)
        dev.run_mcmc(p0s, 40)
        got = dev.get_summary(discard=4, thin=3)
        assert got['quantiles'].shape == (3, 6, 3) and got['count'].shape == (3,)
        for k in range(3):
            want = _host_summary(dev.get_chain(k, discard=4, thin=3, flat=True))
            _same({name: v[k] for name, v in got.items()}, want)
        _same(dev.get_summary(k=1, discard=4, thin=3), {name: v[1] for name, v in got.items()})
        out[mode] = got
    _same(out['device'], out['host'])
    grp.close()


def test_refusals_leave_the_series_usable():
    from mcmc_spec_amd import _lib
    x = np.random.default_rng(2).normal(size=(40, 4, 2))
    ser = _series(x)
    good = ser.order_stats(40, 0, 1, [0], [[0, 159]])
    edges = np.linspace(-1, 1, 5)[None, None, :]
    bad = [lambda: ser.order_stats(41, 0, 1, [0], [[0]]),                    # n > rows
           lambda: ser.order_stats(40, 40, 1, [0], [[0]]),                   # n' = 0
           lambda: ser.order_stats(40, 0, 1, [0], [[160]]),                  # a rank of N
           lambda: ser.order_stats(40, 0, 1, [0], [[-1]]),
           lambda: ser.order_stats(40, 0, 1, [2], [[0]]),                    # a column >= ndim
           lambda: ser.order_stats(40, 0, 1, [_lib.col_ratio(0, 2)], [[0]]),
           lambda: ser.hist(40, 0, 1, [2], edges),
           lambda: ser.hist(41, 0, 1, [0], edges),
           lambda: ser.hist(40, 0, 1, [0], edges[:, :, :1]),                 # nedges = 1
           lambda: ser.hist(40, 0, 1, [0], np.linspace(0, 1, 4098)[None, None, :]),
           lambda: ser.hist(40, 0, 1, [0], edges[:, :, ::-1]),               # descending edges
           lambda: ser.hist2d(40, 0, 1, [(0, 1)], edges[:, :, ::-1], edges),
           lambda: ser.hist2d(40, 0, 1, [(0, 2)], edges, edges),
           lambda: ser.hist2d(40, 40, 1, [(0, 1)], edges, edges)]
    for i, call in enumerate(bad):
        with pytest.raises(ValueError):
            call()
        again = ser.order_stats(40, 0, 1, [0], [[0, 159]])
        assert np.array_equal(again[0], good[0]), i
    assert good[0][0, 0, 0] == x[:, :, 0].min() and good[0][0, 0, 1] == x[:, :, 0].max()
    assert ser.hist(40, 0, 1, [0], edges).sum() == np.sum((x[:, :, 0] >= -1) & (x[:, :, 0] <= 1))
    ser.close()
