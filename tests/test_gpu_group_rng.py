"""GPU: device-drawn randomness for a target group's resident sampler (msx_group_sampler_enqueue_drawn, group_draw_kernel;
mcmc_spec_amd.group.DeviceGroupSampler(rng='device')).  Target k's chain must be, bit for bit, the chain the HOST loop walks
over target k alone when it is fed the device generator's own numbers for k's seed (msx_sampler_draw) -- whatever the
members' walker counts and active starts, across chunk boundaries, runs and reset()."""
import os

import numpy as np
import pytest

from common import golden_case
from test_gpu_group_chain import spread
from test_gpu_target_group import _stage, mixed_engines

pytestmark = pytest.mark.gpu

A = 2.0


def dev_seed(seed):
    return int(seed) & 0xffffffffffffffff


def twin_draws(eng, seed, n, ndim):
    return lambda i, m: eng.ctx.sampler_draw(dev_seed(seed), A, i, m, n, ndim)


def twin(eng, seed, n, ndim, mode='logposterior'):
    """Target k's host twin: the host loop over k's engine alone, fed the device generator's stream of k's seed."""
    from mcmc_spec_amd.sampler import EnsembleSampler
    fn = eng.logposterior if mode == 'logposterior' else eng.loglikelihood
    return EnsembleSampler(n, ndim, fn, vectorize=True, draws=twin_draws(eng, seed, n, ndim))


def same(dev, k, es):
    assert np.array_equal(dev.get_chain(k), es.get_chain()), k
    assert np.array_equal(dev.get_log_prob(k), es.get_log_prob()), k
    assert np.array_equal(dev.acceptance_fraction[k], es.acceptance_fraction), k


def test_each_target_walks_its_own_device_drawn_chain():
    """12 walkers: the smallest ensemble (6 active: a fraction of a wave, the sort padded to 16); 50: 25 active, odd; 258:
    pads to 512, several elements per thread in the sort; 514: 257 active, the output loop strides, pads to 1024.  Active
    starts 0, 6, 31, 160."""
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    c, engines = mixed_engines('B')
    members = engines[:4]
    counts, seeds, n = [12, 50, 258, 514], [2**63 + 41, 42, 43, 44], 7
    p0s = [spread(c, counts[k], 500 + k) for k in range(4)]
    grp = TargetGroup(members)
    dev = DeviceGroupSampler(counts, 6, grp, seeds=seeds, chunk=3, rng='device')
    dev.run_mcmc(p0s, n)
    for k, eng in enumerate(members):
        assert dev.get_chain(k).shape == (n, counts[k], 6)
        es = twin(eng, seeds[k], counts[k], 6)
        es.run_mcmc(p0s[k], n)
        same(dev, k, es)
    assert np.mean([a.mean() for a in dev.acceptance_fraction]) > 0.05
    solo = DeviceEnsembleSampler(50, 6, members[1], rng='device', seed=seeds[1], overlap=False)
    solo.run_mcmc(p0s[1], n)
    same(dev, 1, solo)
    grp.close()


def test_triples_in_likelihood_mode():
    """ndim 8 (zfac = 7 ln z), counts (16, 50); the ensemble of test_mixed_members_and_unequal_walker_counts: tight, the
    companions 100 K above the table's lower end, so that the few iterations stay on the tables."""
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    c, engines = mixed_engines('C')
    members = engines[:2]
    counts, seeds, n = [16, 50], [300, 301], 7
    p0s = [spread(c, counts[k], 500 + k, 0.1) for k in range(2)]
    for p in p0s:
        p[:, 1:c.nspec] += 100.0
    grp = TargetGroup(members)
    dev = DeviceGroupSampler(counts, 8, grp, mode='loglikelihood', seeds=seeds, chunk=3, rng='device')
    dev.run_mcmc(p0s, n)
    for k, eng in enumerate(members):
        es = twin(eng, seeds[k], counts[k], 8, 'loglikelihood')
        es.run_mcmc(p0s[k], n)
        same(dev, k, es)
    grp.close()


def test_runs_continue_and_reset_does_not_rewind():
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    c, engines = mixed_engines('B')
    members = engines[:3]
    counts, seeds = [16, 24, 50], [7, 8, 9]
    p0s = [spread(c, n, 40 + k) for k, n in enumerate(counts)]
    grp = TargetGroup(members)
    dev = DeviceGroupSampler(counts, 6, grp, seeds=seeds, chunk=4, rng='device')
    st = dev.run_mcmc(p0s, 5)
    dev.reset()
    assert [s._drawn for s in dev.samplers] == [5, 5, 5]
    dev.run_mcmc(st, 6)
    fresh = DeviceGroupSampler(counts, 6, grp, seeds=seeds, chunk=4, rng='device')   # (would replay iterations 0..5)
    fresh.run_mcmc(st, 6)
    for k, eng in enumerate(members):
        es = twin(eng, seeds[k], counts[k], 6)
        s = es.run_mcmc(p0s[k], 5)
        assert np.array_equal(st[k].coords, s.coords) and np.array_equal(st[k].log_prob, s.log_prob), k
        es.reset()
        es.run_mcmc(s, 6)
        assert dev.get_chain(k).shape == (6, counts[k], 6)
        same(dev, k, es)
        assert not np.array_equal(dev.get_chain(k), fresh.get_chain(k)), k
    grp.close()


def test_the_generators_capacity_next_to_the_smallest_ensemble():
    """4096 walkers -- the whole LDS sort, 16 elements per thread -- beside 12."""
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    c, engines = mixed_engines('B')
    members = engines[:2]
    counts, seeds, n = [4096, 12], [5, 6], 2
    p0s = [spread(c, counts[k], 90 + k) for k in range(2)]
    grp = TargetGroup(members)
    dev = DeviceGroupSampler(counts, 6, grp, seeds=seeds, chunk=2, rng='device')
    dev.run_mcmc(p0s, n)
    for k, eng in enumerate(members):
        es = twin(eng, seeds[k], counts[k], 6)
        es.run_mcmc(p0s[k], n)
        same(dev, k, es)
    grp.close()


def _files(d):
    return {name: open(os.path.join(d, name), 'rb').read() for name in sorted(os.listdir(d))}


@pytest.mark.parametrize('autocorr,scale', [('host', 1.0), ('device', 0.1), ('device', 1.0)])
def test_the_protocol_end_to_end(tmp_path, autocorr, scale):
    """run_group_protocol (burn-in, reset, production) on the device-drawn sampler against the same driver on the host twin
    GroupSampler(draws=...).  The samples and every coordinate dump are identical in every case.  The autocorr lines
    (str(mean tau), one per check):
      * autocorr='host': both sides compute tau on the host -- identical files, from the wide ensemble;
      * autocorr='device', a tight ensemble (every walker moves before the first check): the device's direct sums against
        the host's FFT, 1e-9 relative -- what DESIGN.md section 12 promises and tests/test_gpu_autocorr.py asks, and the
        one place where this test asks less than byte equality;
      * autocorr='device', the wide ensemble: target 1's walker 5 does not move in the first check's 11 rows.  For a
        constant series the device gives autocorrelation 1 at every lag (its variance is exactly 0) while the host's
        FFT normalises the rounding residue of x - mean(x) and gets (n - k) / n: section 12's behaviour, independent of who
        draws.  Pinned here: checks whose rows hold no motionless walker agree to 1e-9, the others are finite on both
        sides, at least one such check occurs, and the samples do not depend on it."""
    from mcmc_spec_amd.group import DeviceGroupSampler, GroupSampler, TargetGroup, run_group_protocol
    c, engines = mixed_engines('B')
    members = engines[:2]
    counts, seeds = [16, 16], [21, 22]
    p0s = [spread(c, 16, 70 + k, scale) for k in range(2)]
    grp = TargetGroup(members)
    dev = DeviceGroupSampler(counts, 6, grp, seeds=seeds, chunk=16, rng='device', autocorr=autocorr)
    got = run_group_protocol(dev, [p.copy() for p in p0s], 4, 40, nthin=10, dirname=str(tmp_path / 'dev'))
    host = GroupSampler(counts, 6, grp.logposterior, draws=[twin_draws(members[k], seeds[k], 16, 6) for k in range(2)])
    want = run_group_protocol(host, [p.copy() for p in p0s], 4, 40, nthin=10, dirname=str(tmp_path / 'host'))
    motionless_checks = 0
    for k in range(2):
        assert got[k].shape == (16 * 40, 6) and np.array_equal(got[k], want[k]), k
        g, w = _files(str(tmp_path / 'dev' / 'run{}'.format(k))), _files(str(tmp_path / 'host' / 'run{}'.format(k)))
        assert sorted(g) == sorted(w) and 'samples.txt' in w and 'run{}_autocorr.txt'.format(k) in w
        for name in w:
            if not name.endswith('_autocorr.txt') or autocorr == 'host':
                assert g[name] == w[name], name
                continue
            gv, wv = (np.array([float(v) for v in x[name].split()]) for x in (g, w))
            assert gv.shape == wv.shape == (4,) and np.isnan(gv[0]) and np.isnan(wv[0])   # checks at n = 0, 10, 20, 30
            x = host.get_chain(k)
            for i, n in enumerate((10, 20, 30), start=1):
                rows = x[:n + 1]
                if np.any(np.all(rows == rows[0], axis=(0, 2))):
                    motionless_checks += 1
                    assert np.isfinite(gv[i]) and np.isfinite(wv[i]), (name, n)
                else:
                    assert np.isclose(gv[i], wv[i], rtol=1e-9, atol=0), (name, n, gv[i], wv[i])
    if autocorr == 'device':
        assert (motionless_checks > 0) == (scale == 1.0)
    grp.close()


@pytest.mark.parametrize('rng', ['host', 'device'])
def test_run_mcmc_by_chunks_is_sample_by_iterations(rng):
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    c, engines = mixed_engines('B')
    members = engines[:3]
    counts, seeds = [16, 24, 50], [31, 32, 33]
    p0s = [spread(c, n, 60 + k) for k, n in enumerate(counts)]
    grp = TargetGroup(members)
    by_chunk = DeviceGroupSampler(counts, 6, grp, seeds=seeds, chunk=4, rng=rng)
    ret = by_chunk.run_mcmc(p0s, 11)
    by_iter = DeviceGroupSampler(counts, 6, grp, seeds=seeds, chunk=4, rng=rng)
    nyield, states = 0, None
    for states in by_iter.sample(p0s, 11):
        nyield += 1
    assert nyield == 11 and len(ret) == 3
    for k in range(3):
        assert by_chunk.get_chain(k).shape == (11, counts[k], 6)
        assert np.array_equal(by_chunk.get_chain(k), by_iter.get_chain(k)), k
        assert np.array_equal(by_chunk.get_log_prob(k), by_iter.get_log_prob(k)), k
        assert np.array_equal(by_chunk.acceptance_fraction[k], by_iter.acceptance_fraction[k]), k
        assert by_chunk.samplers[k].iteration == by_iter.samplers[k].iteration == 11
        for a, b in ((ret[k], states[k]), (by_chunk.samplers[k].get_last_sample(), by_iter.samplers[k].get_last_sample())):
            assert np.array_equal(a.coords, b.coords) and np.array_equal(a.log_prob, b.log_prob), k
        assert np.array_equal(ret[k].coords, by_chunk.get_chain(k)[-1])
    grp.close()


def test_refusals_through_the_abi_and_mixed_chunks():
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd.group import TargetGroup
    c = golden_case('B')
    engs = [Engine(0), Engine(0)]
    for e in engs:
        e.stage_specs(c.specs)
        _stage(e, c)
    grp = TargetGroup(engs)
    g = grp.group
    counts, seeds = [16, 24], [11, 12]
    p0 = np.concatenate([spread(c, 16, 1), spread(c, 24, 2)])
    lp = np.concatenate(grp.logposterior([p0[:16], p0[16:]]))

    g.sampler_begin(_lib.MODE_LOGPOST, p0, lp, counts, 2)
    for kw in (dict(a=1.0, first_iter=0), dict(a=float('nan'), first_iter=0), dict(a=2.0, first_iter=-1)):
        with pytest.raises(_lib.MsxError) as ei:
            g.sampler_enqueue_drawn(0, 2, seeds, **kw)
        assert ei.value.code == _lib.MSX_ERR_INVALID, kw
    assert g.lib.msx_group_sampler_enqueue_drawn(g.h, 0, 2, None, 2.0, 0) == _lib.MSX_ERR_INVALID   # seeds NULL
    with pytest.raises(_lib.MsxError) as ei:   # (the chunk length is checked as the host-fed entry checks it)
        g.sampler_enqueue_drawn(0, 3, seeds, 2.0, 0)
    assert ei.value.code == _lib.MSX_ERR_INVALID
    # nothing was queued: the slot is free and the run takes a valid chunk, then the next one
    g.sampler_enqueue_drawn(0, 2, seeds, 2.0, 0)
    g.sampler_enqueue_drawn(1, 2, seeds, 2.0, 2)
    with pytest.raises(_lib.MsxError, match='not collected'):
        g.sampler_enqueue_drawn(0, 2, seeds, 2.0, 4)
    drawn = [g.sampler_collect(s, 2) for s in (0, 1)]
    g.sampler_end()
    assert not drawn[0][3].any() and not drawn[1][3].any()

    # a host-fed chunk, then a drawn one, in one run: fed the generator's own numbers for iterations 0 and 1 (member-local
    # indices, the members' halves side by side), the run is the all-drawn run
    g.sampler_begin(_lib.MODE_LOGPOST, p0, lp, counts, 2)
    parts = [engs[m].ctx.sampler_draw(seeds[m], 2.0, 0, 2, counts[m], 6) for m in range(2)]
    g.sampler_enqueue(0, *[np.concatenate(x, axis=2) for x in zip(*parts)])
    g.sampler_enqueue_drawn(1, 2, seeds, 2.0, 2)
    mixed = [g.sampler_collect(s, 2) for s in (0, 1)]
    coords, logp = g.sampler_end(want_state=True)
    for d, m in zip(drawn, mixed):
        assert np.array_equal(d[0], m[0]) and np.array_equal(d[1], m[1]) and np.array_equal(d[2], m[2])
    assert np.array_equal(coords, drawn[1][0][-1]) and np.array_equal(logp, drawn[1][1][-1])
    assert 0 < drawn[1][2].sum() < 4 * 40 and not np.array_equal(drawn[0][0][0], drawn[1][0][-1])
    grp.close()
