"""GPU: target groups (include/msx.h, msx_group_*; mcmc_spec_amd/group.py) -- the walkers of several staged targets in one
launch.  Walker i of member k must give the bits and the status member k's own launch gives it, in every mode, whatever
the members' pixel counts, bands, priors, grids and walker counts; the lock-step sampler must walk each target's own
chain."""
import numpy as np
import pytest

import common
from common import golden_case, rel_err

pytestmark = pytest.mark.gpu

TIGHT = 1e-9
MODES = ('LOGLIKE', 'LOGPOST', 'CHISQ', 'LOGPRIOR')


def _mode(name):
    from mcmc_spec_amd import _lib
    return getattr(_lib, 'MODE_' + name)


def _stage(eng, c, data=None, err=None, **kw):
    from mcmc_spec_amd import bands
    kw.setdefault('rad_prior', c.nspec == 3)
    data = c.data if data is None else data
    err = c.err if err is None else err
    eng.stage_problem(data, err, c.fr, [min(data[0]), max(data[0])], c.ctm, c.ptm, c.tmi, c.tma, c.matrix, nspec=c.nspec,
                      bands=bands.make_bands(c.tables, *c.vega), av_table=common.av_table_exact(), tmin=c.tmin,
                      tmax=c.tmax, prior=c.prior, **kw)


def koi_engines():
    """The ten KOI cases of tests/golden/golden_koi.npz (eight targets + two wide crops), one Engine each, staged as
    tests/test_koi_config5.py stages them."""
    from mcmc_spec_amd import bands
    from mcmc_spec_amd.engine import Engine
    from test_koi_config5 import koi_cases, koi_problem
    if 'group_koi' not in common._cache:
        g, tags = koi_cases()
        c = golden_case('A')
        bl = bands.make_bands(c.tables, *c.vega)
        engines = []
        for tag in tags:
            data, err, fr, r, ctm, ptm, tmi, tma = koi_problem(g, tag)
            eng = Engine(0)
            eng.stage_specs(c.specs)
            eng.stage_problem(data, err, fr, r, ctm, ptm, tmi, tma, c.matrix, nspec=2, bands=bl,
                              av_table=common.av_table_exact(), tmin=c.tmin, tmax=c.tmax, prior=c.prior, rad_prior=True)
            engines.append(eng)
        common._cache['group_koi'] = (g, tags, engines)
    return common._cache['group_koi']


def mixed_engines(which):
    """Members that differ in every way a group allows: golden case `which` ('B' binary, 'C' triple) as it is, cropped to
    fewer pixels, with dist_fit False, use_av False, without the spectrum term, on a grid missing one node, and on a
    component grid rotated differently per star; plus (binaries) golden case A (no photometry, 2,064-pixel synthetic file)."""
    from mcmc_spec_amd.engine import Engine
    key = ('group_mixed', which)
    if key in common._cache:
        return common._cache[key]
    c = golden_case(which)
    out = []

    def add(specs=None, **kw):
        eng = Engine(0)
        eng.stage_specs(c.specs if specs is None else specs)
        _stage(eng, c, **kw)
        out.append(eng)
        return eng
    add()
    n = len(c.data[0]) // 2 + 37
    add(data=[np.asarray(c.data[0])[:n], np.asarray(c.data[1])[:n]], err=np.asarray(c.err)[:n])
    add(dist_fit=False)
    add(use_av=False)
    add(spectrum=False)
    specs = dict(c.specs)
    del specs['3800, 5.0']
    add(specs=specs)
    rot = Engine(0)
    rot.stage_specs(c.specs)
    wl_um = np.asarray(c.data[0])
    win = [np.floor(wl_um.min() * 1e4) - 20.0, np.ceil(wl_um.max() * 1e4) + 20.0]
    rot.broaden_grid_window(win, 1700, vsini=(40.0, 12.0, 25.0)[:c.nspec], limb=(0.6, 0.3, 0.5)[:c.nspec])
    _stage(rot, c)
    out.append(rot)
    if which == 'B':
        a = golden_case('A')
        eng = Engine(0)
        eng.stage_specs(a.specs)
        _stage(eng, a)
        out.append(eng)
    common._cache[key] = (c, out)
    return common._cache[key]


def edge_walkers(c, n, seed):
    """n walkers around the golden thetas, a quarter moved far (outside the grid, the isochrone or the prior box), with
    the error patterns of tests/test_gpu_parity.py::test_error_conventions planted among them."""
    rng = np.random.default_rng(seed)
    base = np.tile(c.theta, (n // len(c.theta) + 1, 1))[:n].copy()
    ns = c.nspec
    sc = np.array([15.0] * ns + [0.01] + [0.01] * ns + [1e-5])
    th = base + rng.normal(size=base.shape) * sc * (rng.random((n, 1)) < 0.75)
    far = rng.random(n) < 0.25
    th[far, :ns] = rng.uniform(2600.0, 4600.0, size=(far.sum(), ns))
    for i in range(0, n, 9):
        th[i, 1] = 2800.0                  # outside the isochrone: ValueError (likelihood), reject (posterior)
    for i in range(4, n, 11):
        th[i, 0], th[i, 1] = 4325.0, 3500.0  # beyond the last node: IndexError
    return th


def solo(eng, th, mode):
    return eng.ctx.logprob_batch(th, _mode(mode))


def check_group_equals_members(grp, engines, ths, modes=MODES):
    """One group launch per mode against each member's own launch: same bits, same statuses."""
    counts = [len(t) for t in ths]
    flat = np.concatenate(ths) if sum(counts) else np.empty((0, engines[0].ndim))
    seen = set()
    for mode in modes:
        lp, st = grp.group.logprob_batch(flat, counts, _mode(mode))
        o = 0
        for k, (eng, th) in enumerate(zip(engines, ths)):
            if len(th):
                want_lp, want_st = solo(eng, th, mode)
                assert np.array_equal(lp[o:o + len(th)], want_lp, equal_nan=True), (mode, k)
                assert np.array_equal(st[o:o + len(th)], want_st), (mode, k)
                seen |= set(int(s) for s in want_st)
            o += len(th)
    return seen


def test_koi_targets_in_one_launch_match_the_fixture_and_their_own_launches():
    from mcmc_spec_amd.group import TargetGroup
    g, tags, engines = koi_engines()
    grp = TargetGroup(engines)
    ths = [g['theta']] * len(engines)
    check_group_equals_members(grp, engines, ths)
    ll = grp.loglikelihood(ths)
    lpo = grp.logposterior(ths)
    for k, tag in enumerate(tags):
        assert rel_err(ll[k], g[tag + '_loglike']).max() < TIGHT, tag
        assert rel_err(lpo[k], g[tag + '_logpost']).max() < TIGHT, tag
    info = grp.launch_info([16] * len(engines))
    assert info['kernel'].startswith('logprob_group_kernel<NS=2') and info['workgroups'] == 16 * len(engines)


@pytest.mark.parametrize('which', ['B', 'C'])
def test_mixed_members_give_their_own_bits_and_statuses(which):
    from mcmc_spec_amd.group import TargetGroup
    c, engines = mixed_engines(which)
    grp = TargetGroup(engines)
    ths = [edge_walkers(c, 40 + 13 * k, seed=100 * k + 7) for k in range(len(engines))]
    seen = check_group_equals_members(grp, engines, ths)
    from mcmc_spec_amd import _lib
    assert {_lib.W_OK, _lib.W_REJECT, _lib.W_KEYERROR, _lib.W_INDEXERROR, _lib.W_VALUEERROR} <= seen, seen
    # per-walker errors raise what Engine raises, naming the target
    k_missing = 5
    bad = [np.empty((0, c.nspec * 2 + 2))] * len(engines)
    bad[k_missing] = c.theta[:1]
    with pytest.raises(KeyError, match='target {}'.format(k_missing)):
        grp.loglikelihood(bad)
    grp.close()


def test_shapes_block_sizes_and_empty_members():
    import torch
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.group import TargetGroup
    c, engines = mixed_engines('B')
    grp = TargetGroup(engines)
    K = len(engines)
    stream = torch.cuda.current_stream().cuda_stream
    layouts = [[1] + [0] * (K - 1), [0, 0, 3] + [0] * (K - 3), [5, 0, 17, 0, 1, 64, 0, 2][:K] + [0] * (K - 8),
               [300, 0, 700, 64, 0, 1200, 900, 1000][:K] + [0] * (K - 8)]
    for li, counts in enumerate(layouts):
        ths = [edge_walkers(c, n, seed=31 * li + k) if n else np.empty((0, 6)) for k, n in enumerate(counts)]
        flat = np.concatenate(ths)
        want = [solo(e, t, 'LOGPOST') if len(t) else (np.empty(0), np.empty(0, np.int32)) for e, t in zip(engines, ths)]
        want_lp = np.concatenate([w[0] for w in want])
        want_st = np.concatenate([w[1] for w in want])
        d_th = torch.from_numpy(flat).cuda()
        for block in (0, 256, 512, _lib.BLOCK_512_SHARED):
            d_lp = torch.full((len(flat),), 7.0, dtype=torch.float64, device='cuda')
            d_st = torch.full((len(flat),), -9, dtype=torch.int32, device='cuda')
            grp.group.logprob_batch_dev(d_th.data_ptr(), counts, 6, d_lp.data_ptr(), d_st.data_ptr(), stream,
                                        mode=_lib.MODE_LOGPOST, block_threads=block)
            torch.cuda.synchronize()
            assert np.array_equal(d_lp.cpu().numpy(), want_lp, equal_nan=True), (counts, block)
            assert np.array_equal(d_st.cpu().numpy(), want_st), (counts, block)
    assert sum(layouts[-1]) > 4096
    # no walkers at all: nothing launched, nothing raised
    assert [len(x) for x in grp.logposterior([np.empty((0, 6))] * K)] == [0] * K
    grp.close()


def test_refusals():
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.engine import Engine
    from mcmc_spec_amd.group import TargetGroup
    c, engines = mixed_engines('B')
    c3, triples = mixed_engines('C')
    with pytest.raises(ValueError, match='member 1 has nspec'):
        TargetGroup([engines[0], triples[0]])
    f32 = Engine(0)
    f32.stage_specs(c.specs)
    _stage(f32, c, store='f32')
    with pytest.raises(_lib.MsxError, match='member 2 .*float32'):
        TargetGroup([engines[0], engines[1], f32])
    # a member over 17,152 pixels (the bench workload's config 4 spectrum)
    from bench import build_workload
    big = Engine(0)
    build_workload(big, 17408, False)
    with pytest.raises(ValueError, match='member 1 has 17408 pixels'):
        TargetGroup([engines[0], big])
    # restaged member: refused at the next launch, naming it
    a, b = Engine(0), Engine(0)
    for e in (a, b):
        e.stage_specs(c.specs)
        _stage(e, c)
    grp = TargetGroup([a, b])
    th = [c.theta[:2], c.theta[:3]]
    grp.logposterior(th)
    _stage(b, c)
    with pytest.raises(_lib.MsxError, match='member 1.*staged again'):
        grp.logposterior(th)
    grp.close()
    # destroyed member: refused, never read
    grp = TargetGroup([a, b])
    grp.logposterior(th)
    a.ctx.close()
    with pytest.raises(_lib.MsxError, match='member 0 was destroyed'):
        grp.logposterior(th)
    grp.close()


def test_group_sampler_walks_each_targets_own_chain():
    from mcmc_spec_amd import synth
    from mcmc_spec_amd.group import GroupSampler, TargetGroup
    from mcmc_spec_amd.sampler import EnsembleSampler
    g, tags, engines = koi_engines()
    c = golden_case('A')
    members = engines[:4]
    grp = TargetGroup(members)
    seeds = [11, 12, 13, 14]
    p0s = [synth.draw_walkers(32, seed=40 + k, tmin=c.tmin, tmax=c.tmax) for k in range(4)]
    gs = GroupSampler([32] * 4, 6, grp.logposterior, seeds=seeds)
    gs.run_mcmc(p0s, 20)
    for k, eng in enumerate(members):
        es = EnsembleSampler(32, 6, eng.logposterior, vectorize=True, seed=seeds[k])
        es.run_mcmc(p0s[k], 20)
        assert np.array_equal(gs.get_chain(k), es.get_chain()), k
        assert np.array_equal(gs.get_log_prob(k), es.get_log_prob()), k
        assert np.array_equal(gs.acceptance_fraction[k], es.acceptance_fraction), k
    assert np.mean([a.mean() for a in gs.acceptance_fraction]) > 0.05
