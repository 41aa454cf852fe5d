"""GPU: the device chain series and the autocorrelation time computed from it (include/msx.h, msx_series_*; DESIGN.md
section 12; mcmc_spec_amd.sampler / group, autocorr='device').  The rows the runs append must be the host chain bit for
bit whatever the chunking, breaks, growth, overlap or sharding; f must match a direct-sum restatement and the host's FFT;
tau must match the host method with the same window; the protocols must stop where the host's stop."""
import os

import numpy as np
import pytest

from autocorr_numpy import acf_direct, acf_fft_host, ar1, assert_not_borderline
from common import golden_case
from test_gpu_parity import make_engine

pytestmark = pytest.mark.gpu


def _eng():
    import common
    if 'autocorr_engA' not in common._cache:
        common._cache['autocorr_engA'] = make_engine(golden_case('A'))
    return common._cache['autocorr_engA']


def _p0(nw, seed=3):
    from mcmc_spec_amd import synth
    c = golden_case('A')
    return synth.draw_walkers(nw, seed=seed, tmin=c.tmin, tmax=c.tmax)


def _held(s):
    """The rows the sampler's series holds for its stored chain, next to that chain."""
    n = len(s._chain)
    return s._series.read(0, n), np.array(s._chain)


def _host_tau(chain, **kw):
    from mcmc_spec_amd.sampler import EnsembleSampler
    h = EnsembleSampler(chain.shape[1], chain.shape[2], None, vectorize=True, seed=0)
    h._chain = list(chain)
    return h.get_autocorr_time(**kw)


@pytest.mark.parametrize('overlap', [None, False])
def test_rows_are_the_host_chain_through_breaks_store_false_reset_and_growth(overlap):
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    eng = _eng()
    s = DeviceEnsembleSampler(64, 6, eng, seed=5, chunk=8, overlap=overlap, autocorr='device')
    st = s.run_mcmc(_p0(64), 29)                       # chunk 8, a ragged last chunk
    got, want = _held(s)
    assert np.array_equal(got, want)
    if overlap is None:
        assert s.overlapped
    for i, st in enumerate(s.sample(st, iterations=40)):   # a consumer that breaks mid-chunk
        if i == 12:
            break
    st = s.run_mcmc(st, 10, store=False)               # store=False in between: nothing appended
    st = s.run_mcmc(st, 21)
    got, want = _held(s)
    assert len(want) == 29 + 13 + 21 and np.array_equal(got, want)
    s.reset()
    st = s.run_mcmc(st, 11)
    got, want = _held(s)
    assert len(want) == 11 and np.array_equal(got, want)
    # growth (the first buffer holds 256 rows), with get_autocorr_time and reads while chunks are in flight
    for i, st in enumerate(s.sample(st, iterations=600)):
        n = len(s._chain)
        if n in (250, 262, 300, 513, 611):
            tau = s.get_autocorr_time(quiet=True)
            chain = np.array(s._chain)
            assert np.array_equal(s._series.read(0, n), chain), n
            f = s._series.acf(n, nlag=min(n, 320))
            assert np.max(np.abs(f - acf_direct(chain, n, nlag=min(n, 320)))) < 1e-12, n
            h = _host_tau(chain, quiet=True)
            assert np.allclose(tau, h, rtol=1e-9, atol=0), (n, tau, h)
    got, want = _held(s)
    assert len(want) == 611 and np.array_equal(got, want)


def test_rows_of_a_sharded_run_with_world_one():
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    eng = _eng()
    s = DeviceEnsembleSampler(32, 6, eng, seed=9, chunk=6, shard=(0, 1), autocorr='device')
    s.run_mcmc(_p0(32, 4), 23)
    got, want = _held(s)
    assert np.array_equal(got, want)


@pytest.mark.parametrize('rho', [0.5, 0.9, 0.99])
def test_f_matches_the_direct_sum_and_the_host_fft(rho):
    """AR(1) rows up to 15,000, one walker stuck at 0.5 (mean exact on both sides: ones), discard / thin, three members."""
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.engine import Engine
    ctx = _eng().ctx
    n, nw, ndim = 15000, 20, 3
    x = ar1(n, nw, ndim, rho, seed=int(rho * 1000))
    x[:, 7, 1] = 0.5
    counts = [5, 11, 4]
    ser = _lib.Series(ctx, nw, ndim, counts)
    ser.append(x[:4000])
    ser.append(x[4000:])
    assert ser.rows == n
    for (nn, disc, thin, lag0, nlag) in [(n, 0, 1, 0, 640), (n, 0, 1, 900, 500), (9001, 123, 3, 0, 700), (n, 0, 1, 0, 4)]:
        f = ser.acf(nn, disc, thin, lag0, nlag)
        want = acf_direct(x, nn, disc, thin, lag0, nlag, counts)
        assert np.max(np.abs(f - want)) <= 1e-12, (nn, disc, thin, lag0, np.max(np.abs(f - want)))
        fft = acf_fft_host(x, nn, disc, thin, counts)[:, :, lag0:lag0 + nlag]
        assert np.max(np.abs(f - fft)) <= 1e-12, (nn, disc, thin, lag0, np.max(np.abs(f - fft)))
    f = ser.acf(n, nlag=10, dims=[1])
    assert np.all(np.isnan(f[:, [0, 2]])) and np.array_equal(f[:, 1], ser.acf(n, nlag=10)[:, 1])
    ser.close()


def test_tau_of_sampled_chains_matches_the_host():
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    eng = _eng()
    s = DeviceEnsembleSampler(50, 6, eng, seed=21, chunk=32, autocorr='device')
    s.run_mcmc(_p0(50, 8), 700)
    chain = np.array(s._chain)
    for kw in ({}, {'discard': 100, 'thin': 3}):
        assert_not_borderline(acf_fft_host(chain, len(chain), kw.get('discard', 0), kw.get('thin', 1))[0])
        got = s.get_autocorr_time(quiet=True, **kw)
        want = _host_tau(chain, quiet=True, **kw)
        assert np.allclose(got, want, rtol=1e-9, atol=0), (kw, got, want)


def _group_case(kind):
    from mcmc_spec_amd import synth
    from test_gpu_group_chain import spread
    from test_gpu_target_group import koi_engines, mixed_engines
    if kind == 'koi':
        members = koi_engines()[2][:8]
        c = golden_case('A')
        counts = [50] * 8
        return members, 6, counts, [synth.draw_walkers(50, seed=70 + k, tmin=c.tmin, tmax=c.tmax) for k in range(8)]
    c, engines = mixed_engines(kind)
    members = engines[:5] + engines[6:]
    counts = [(16, 24, 50, 64)[k % 4] for k in range(len(members))]
    return members, 2 * c.nspec + 2, counts, [spread(c, counts[k], 500 + k) for k in range(len(members))]


@pytest.mark.parametrize('kind', ['koi', 'B', 'C'])
def test_group_tau_matches_each_targets_host_tau(kind):
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    members, ndim, counts, p0s = _group_case(kind)
    grp = TargetGroup(members)
    dev = DeviceGroupSampler(counts, ndim, grp, seeds=[40 + k for k in range(len(members))], chunk=16, autocorr='device')
    dev.run_mcmc(p0s, 300)
    tau = dev.get_autocorr_time(quiet=True)
    assert tau.shape == (len(members), ndim)
    for k in range(len(members)):
        chain = dev.get_chain(k)
        assert np.array_equal(dev._series.read(0, 300)[:, sum(counts[:k]):sum(counts[:k + 1])], chain)
        assert_not_borderline(acf_fft_host(chain, 300)[0])
        want = _host_tau(chain, quiet=True)
        assert np.allclose(tau[k], want, rtol=1e-9, atol=0), (k, tau[k], want)
        assert np.array_equal(dev.get_autocorr_time(k, quiet=True), tau[k])
    grp.close()


@pytest.mark.parametrize('rho', [0.5, 0.9])
def test_ar1_tau_at_1024_walkers_and_15000_rows(rho):
    """The largest buffer (1,024 x 6 x 15,000 doubles = 737 MB): tau within a few per cent of (1 + rho) / (1 - rho)."""
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.sampler import _device_integrated_time
    n, nw, ndim = 15000, 1024, 6
    ser = _lib.Series(_eng().ctx, nw, ndim)
    rng = np.random.default_rng(int(rho * 10))
    x = rng.normal(size=(nw, ndim))
    s = np.sqrt(1.0 - rho * rho)
    for b in range(0, n, 1000):   # (uploaded in pieces: 1,000 rows = 49 MB)
        blk = np.empty((1000, nw, ndim))
        for t in range(1000):
            x = rho * x + s * rng.standard_normal((nw, ndim))
            blk[t] = x
        ser.append(blk)
    tau = _device_integrated_time(ser, n, 5.0, 0, 1)[0]
    want = (1 + rho) / (1 - rho)
    assert np.all(np.abs(tau / want - 1) < 0.03), (tau, want)
    ser.close()


def test_bits_do_not_depend_on_the_call_the_tiles_or_the_chunking():
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    ctx = _eng().ctx
    x = ar1(5000, 16, 2, 0.95, seed=2)
    a, b = _lib.Series(ctx, 16, 2), _lib.Series(ctx, 16, 2)
    a.append(x)
    for i in range(0, 5000, 7):
        b.append(x[i:i + 7])
    fa = a.acf(5000, 0, 1, 0, 960)
    assert np.array_equal(fa, a.acf(5000, 0, 1, 0, 960)) and np.array_equal(fa, b.acf(5000, 0, 1, 0, 960))
    assert np.array_equal(fa, np.concatenate([a.acf(5000, 0, 1, 0, 320), a.acf(5000, 0, 1, 320, 17), a.acf(5000, 0, 1, 337, 623)], axis=2))
    eng = _eng()
    runs = []
    for chunk in (8, 13):
        s = DeviceEnsembleSampler(32, 6, eng, seed=33, chunk=chunk, autocorr='device')
        s.run_mcmc(_p0(32, 5), 90)
        runs.append((s._series.acf(90), s.get_autocorr_time(quiet=True)))
    assert np.array_equal(runs[0][0], runs[1][0]) and np.array_equal(runs[0][1], runs[1][1])


def _files(d):
    return {name: open(os.path.join(d, name), 'rb').read() for name in sorted(os.listdir(d))}


def _same_files(got, want):
    """Every dump identical; the autocorr lines (str(mean tau)) equal to 1e-9 relative: device and host tau differ in roundoff."""
    assert sorted(got) == sorted(want)
    for name in want:
        if name.endswith('_autocorr.txt'):
            g = np.array([float(v) for v in got[name].split()])
            w = np.array([float(v) for v in want[name].split()])
            assert g.shape == w.shape and np.allclose(g, w, rtol=1e-9, atol=0, equal_nan=True), name
        else:
            assert got[name] == want[name], name


def test_reference_protocol_with_device_checks_stops_where_the_host_checks_stop(tmp_path):
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler, run_reference_protocol
    eng = _eng()
    out = {}
    for mode in ('host', 'device'):
        d = tmp_path / mode
        d.mkdir()
        s = DeviceEnsembleSampler(50, 6, eng, seed=77, chunk=64, autocorr=mode)
        out[mode] = run_reference_protocol(s, _p0(50, 9), 100, 2500, nthin=50, dirname=str(d), fname='t')
    assert np.array_equal(out['device'], out['host'])
    _same_files(_files(str(tmp_path / 'device')), _files(str(tmp_path / 'host')))


def test_group_protocol_on_the_device_is_each_targets_host_protocol(tmp_path):
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup, run_group_protocol
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler, run_reference_protocol
    members, ndim, counts, p0s = _group_case('koi')
    seeds = [60 + k for k in range(8)]
    grp = TargetGroup(members)
    dev = DeviceGroupSampler(counts, ndim, grp, seeds=seeds, chunk=64, autocorr='device')
    fnames = ['koi{}'.format(k) for k in range(8)]
    got = run_group_protocol(dev, [p.copy() for p in p0s], 100, 1500, nthin=50, dirname=str(tmp_path / 'g'), fnames=fnames)
    for k, eng in enumerate(members):
        d = tmp_path / 'solo{}'.format(k)
        d.mkdir()
        solo = DeviceEnsembleSampler(counts[k], ndim, eng, seed=seeds[k], chunk=64)   # (its host method; the host loop's chain)
        want = run_reference_protocol(solo, p0s[k].copy(), 100, 1500, nthin=50, dirname=str(d), fname=fnames[k])
        assert np.array_equal(got[k], want), k
        _same_files(_files(str(tmp_path / 'g' / fnames[k])), _files(str(d)))
    grp.close()
