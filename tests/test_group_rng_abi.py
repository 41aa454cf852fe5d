"""CPU: device-drawn randomness for a target group's resident sampler (include/msx.h, msx_group_sampler_enqueue_drawn;
mcmc_spec_amd.group.DeviceGroupSampler(rng='device')) is declared, exported and mirrored; both draw kernels keep their
working set in registers; GroupSampler(draws=[...]) -- the host twin -- walks each target's own EnsembleSampler(draws=)
chain and carries the absolute iteration across reset().  No compute calls (no GPU here)."""
import ctypes as C
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import common  # noqa: F401
from mcmc_spec_amd import _lib
from mcmc_spec_amd.group import DeviceGroupSampler, GroupSampler
from mcmc_spec_amd.sampler import EnsembleSampler, counter_draws

ROOT = common.ROOT
HDR = os.path.join(ROOT, 'include', 'msx.h')
NAME = 'msx_group_sampler_enqueue_drawn'
NDIM = 6


def test_header_declares_and_library_exports_the_drawn_entry():
    import __graft_entry__ as ge
    ge.build()
    txt = re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)
    m = re.search(r'\bint ' + NAME + r'\s*\(([^)]*)\)\s*;', txt)
    assert m, NAME
    params = [' '.join(p.split()) for p in m.group(1).split(',')]
    assert params == ['msx_group *group', 'int32_t slot', 'int64_t nsteps', 'const uint64_t *seeds', 'double a', 'int64_t first_iter'], params
    lib = _lib.load()
    assert NAME in _lib.EXPORTED
    fn = getattr(lib, NAME)
    assert fn.restype is C.c_int
    assert list(fn.argtypes) == [C.c_void_p, C.c_int32, C.c_int64, C.POINTER(C.c_uint64), C.c_double, C.c_int64]
    assert hasattr(_lib.Group, 'sampler_enqueue_drawn')


def test_draw_kernels_use_no_scratch():
    """sampler_draw_kernel and group_draw_kernel (csrc/logprob_kernel.h): scratch 0 (tests/test_group_chain_abi.py's method)."""
    src = os.path.join(ROOT, 'mcmc_spec_amd', 'csrc', 'msx.hip')
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, 't.s')
        out = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                              '-mllvm', '-amdgpu-kernarg-preload-count=8',
                              '-Rpass-analysis=kernel-resource-usage', '-o', asm, src],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    seen = {'sampler_draw_kernel': 0, 'group_draw_kernel': 0}
    for i, ln in enumerate(lines):
        for name in seen:
            if 'Function Name' in ln and name in ln:
                block = '\n'.join(lines[i:i + 14])
                m = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block)
                assert m and int(m.group(1)) == 0, block
                seen[name] += 1
    assert seen == {'sampler_draw_kernel': 1, 'group_draw_kernel': 1}, seen


# ---- GroupSampler(draws=[...]) ---------------------------------------------------------------------------------------
COUNTS, SEEDS, A = (12, 50, 130), (2**63 + 11, 5, 77), 2.0


def make_target(k):
    rng = np.random.default_rng(100 + k)
    mu, isig = rng.normal(size=NDIM), 1.0 / rng.uniform(0.5, 2.0, size=NDIM)

    def lnp(x):
        x = np.atleast_2d(x)
        return -0.5 * np.sum(((x - mu) * isig) ** 2, axis=1)
    return lnp


def twin_draws(k):
    return lambda i, m: counter_draws(SEEDS[k], A, NDIM, i, m, COUNTS[k])


def group_of_twins(fns):
    return GroupSampler(COUNTS, NDIM, lambda ts: [f(t) for f, t in zip(fns, ts)], a=A, draws=[twin_draws(k) for k in range(len(COUNTS))])


def test_group_sampler_with_draws_walks_each_targets_own_fed_chain():
    fns = [make_target(k) for k in range(3)]
    p0s = [np.random.default_rng(30 + k).normal(size=(n, NDIM)) for k, n in enumerate(COUNTS)]
    gs = group_of_twins(fns)
    gs.run_mcmc(p0s, 9)
    split = group_of_twins(fns)
    st = split.run_mcmc(p0s, 4)
    split.reset()                      # (the chain starts over; the stream does not)
    assert [s._drawn for s in split.samplers] == [4, 4, 4]
    split.run_mcmc(st, 5)
    for k in range(3):
        es = EnsembleSampler(COUNTS[k], NDIM, fns[k], a=A, vectorize=True, draws=twin_draws(k))
        es.run_mcmc(p0s[k], 9)
        assert gs.get_chain(k).shape == (9, COUNTS[k], NDIM)
        assert np.array_equal(gs.get_chain(k), es.get_chain()), k
        assert np.array_equal(gs.get_log_prob(k), es.get_log_prob()), k
        assert np.array_equal(gs.acceptance_fraction[k], es.acceptance_fraction), k
        assert gs.acceptance_fraction[k].mean() > 0.1
        assert np.array_equal(split.get_chain(k), gs.get_chain(k)[4:]), k
        assert np.array_equal(split.get_log_prob(k), gs.get_log_prob(k)[4:]), k
    with pytest.raises(ValueError, match='one draws callable per target'):
        GroupSampler(COUNTS, NDIM, None, draws=[twin_draws(0)])


def test_group_sampler_without_draws_gives_the_chain_it_gave():
    fns = [make_target(k) for k in range(3)]
    seeds = [3, 10, 17]
    p0s = [np.random.default_rng(k).normal(size=(n, NDIM)) for k, n in enumerate(COUNTS)]
    gs = GroupSampler(COUNTS, NDIM, lambda ts: [f(t) for f, t in zip(fns, ts)], seeds=seeds)
    gs.run_mcmc(p0s, 12)
    for k in range(3):
        es = EnsembleSampler(COUNTS[k], NDIM, fns[k], vectorize=True, seed=seeds[k])
        es.run_mcmc(p0s[k], 12)
        assert np.array_equal(gs.get_chain(k), es.get_chain()), k
        assert np.array_equal(gs.get_log_prob(k), es.get_log_prob()), k
        assert np.array_equal(gs.acceptance_fraction[k], es.acceptance_fraction), k


# ---- DeviceGroupSampler's constructor, before anything touches a GPU ------------------------------------------------------
class StubGroup:
    """What DeviceGroupSampler.__init__ reads of a TargetGroup; any call would be a GPU call."""

    def __init__(self, k):
        self.k = k
        self.engines = [None] * k

    def __len__(self):
        return self.k

    def logposterior(self, thetas):
        raise AssertionError('no evaluation at construction')

    loglikelihood = logposterior


def test_device_group_sampler_refuses_unknown_rng_and_too_many_walkers():
    with pytest.raises(ValueError, match='rng'):
        DeviceGroupSampler([16, 16], NDIM, StubGroup(2), seeds=[1, 2], rng='gpu')
    with pytest.raises(ValueError, match='4096'):
        DeviceGroupSampler([16, 4098], NDIM, StubGroup(2), seeds=[1, 2], rng='device')
    # the limit is the device generator's: host-drawn ensembles may be larger, and 4096 is taken
    assert DeviceGroupSampler([16, 4098], NDIM, StubGroup(2), seeds=[1, 2]).rng_mode == 'host'
    s = DeviceGroupSampler([16, 4096], NDIM, StubGroup(2), seeds=[2**64 + 5, np.random.SeedSequence(9)], rng='device')
    assert s.rng_mode == 'device'
    # one device seed per target, derived as DeviceEnsembleSampler.device_seed is
    assert s.device_seeds == [5, int(np.random.SeedSequence(9).generate_state(1, dtype=np.uint64)[0])]
    none = DeviceGroupSampler([16], NDIM, StubGroup(1), rng='device')
    assert len(none.device_seeds) == 1 and 0 <= none.device_seeds[0] < 2**64


def test_design_md_holds_the_generated_group_rng_tables():
    """DESIGN.md section 11.2's tables are what tools/design_tables.py makes of profiles/group_chains_rng.jsonl, and that
    file holds the three shapes the section reports, each meeting the no-regression condition."""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import design_tables as dt
    text = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert dt.GROUP_RNG_BEGIN in text and dt.GROUP_RNG_END in text
    block = text[text.index(dt.GROUP_RNG_BEGIN) + len(dt.GROUP_RNG_BEGIN):text.index(dt.GROUP_RNG_END)]
    assert block.strip() == dt.build_group_rng().strip() and block.strip()
    rows = [json.loads(ln) for ln in open(os.path.join(ROOT, 'profiles', 'group_chains_rng.jsonl')) if ln.startswith('{')]
    shapes = {(r['targets'], r['walkers_per_target']): r for r in rows}
    for shape in ((8, 50), (8, 16), (1, 50)):
        r = shapes[shape]
        assert len(r['device_rounds']) == len(r['device_rng_rounds']) == 5
        assert set(r['device_rng_host_us_per_chunk']) == {'draw_wait', 'enqueue', 'collect', 'states'}
        assert r['no_regression'] == (r['device_rng'] - r['device'] <= max(r['device_rounds']) - min(r['device_rounds']))
        # the issue's one condition: device-drawn no slower than host-drawn by more than the host-drawn driver's own spread
        assert r['no_regression'], (shape, r['device_rng_rounds'], r['device_rounds'])
