"""CPU: the group tempering ABI (include/msx.h, msx_group_tempered_* and msx_group_ladder_*): the nine functions are declared,
exported and mirrored with the right ctypes signatures, the wrappers take what the sampler passes, a null group is refused,
the kernels' header sits where the translation unit needs it and leaves the single-target texts alone.  No GPU here."""
import ctypes as C
import inspect
import os
import re

import common  # noqa: F401
from mcmc_spec_amd import _lib, moves, tempered

ROOT = common.ROOT
HDR = os.path.join(ROOT, 'include', 'msx.h')
CSRC = os.path.join(ROOT, 'mcmc_spec_amd', 'csrc')

I32P, DP, I64P, U64P, VP = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.c_void_p
SETP = C.POINTER(moves.MsxMoveSet)
GENERAL = ['const int32_t *sidx', 'const int32_t *cidx', 'const int32_t *kind', 'const int32_t *p1', 'const int32_t *p2',
           'const double *g', 'const double *fac', 'const double *logu', 'const double *swap_logu']
FUNCTIONS = {
    'msx_group_tempered_begin': (['msx_group *group', 'int32_t ntemps', 'const double *betas', 'const int64_t *counts', 'int32_t ndim',
                                  'int64_t max_chunk_steps', 'const double *coords', 'const double *ll', 'const double *lpr'],
                                 [VP, C.c_int32, DP, I64P, C.c_int32, C.c_int64, DP, DP, DP]),
    'msx_group_tempered_enqueue': (['msx_group *group', 'int32_t slot', 'int64_t nsteps'] + GENERAL,
                                   [VP, C.c_int32, C.c_int64] + [I32P] * 5 + [DP] * 4),
    'msx_group_tempered_enqueue_drawn': (['msx_group *group', 'int32_t slot', 'int64_t nsteps', 'const uint64_t *seeds',
                                          'const msx_move_set *set', 'int64_t first_iter'], [VP, C.c_int32, C.c_int64, U64P, SETP, C.c_int64]),
    'msx_group_tempered_collect': (['msx_group *group', 'int32_t slot', 'double *chain', 'double *ll_chain', 'double *lpr_chain',
                                    'int64_t *naccept', 'int64_t *nswap', 'int32_t *worst'], [VP, C.c_int32, DP, DP, DP, I64P, I64P, I32P]),
    'msx_group_tempered_end': (['msx_group *group', 'double *coords', 'double *ll', 'double *lpr'], [VP, DP, DP, DP]),
    'msx_group_tempered_attach_series': (['msx_group *group', 'msx_series *chain', 'msx_series *dens', 'int64_t at_row'], [VP, VP, VP, C.c_int64]),
    'msx_group_ladder_adapt': (['msx_group *group', 'const double *lag', 'const double *time', 'const int64_t *k0'], [VP, DP, DP, I64P]),
    'msx_group_ladder_betas': (['msx_group *group', 'int32_t slot', 'double *out'], [VP, C.c_int32, DP]),
    'msx_group_ladder_current': (['msx_group *group', 'double *betas', 'int64_t *k', 'int64_t *skipped'], [VP, DP, I64P, I64P]),
}


def header():
    return re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)


def test_the_nine_functions_are_declared_exported_and_mirrored():
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load()
    txt = header()
    for name, (params, argtypes) in FUNCTIONS.items():
        m = re.search(r'\bint ' + name + r'\s*\(([^)]*)\)\s*;', txt)
        assert m, name
        assert [' '.join(p.split()) for p in m.group(1).split(',')] == params, name
        assert name in _lib.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
    family = lambda n: n.startswith(('msx_group_tempered_', 'msx_group_ladder_'))
    assert sorted(n for n in _lib.EXPORTED if family(n)) == sorted(FUNCTIONS)
    assert sorted(set(re.findall(r'\b(msx_group_(?:tempered|ladder)_[a-z_]+)\s*\(', txt))) == sorted(FUNCTIONS)


def test_a_null_group_is_refused_without_a_device():
    """The argument checks that need no device: every entry point returns MSX_ERR_INVALID for a null group."""
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load()
    for name, (_, argtypes) in FUNCTIONS.items():
        args = [None if t in (VP, DP, I64P, I32P, U64P, SETP) else 0 for t in argtypes]
        assert getattr(lib, name)(*args) == _lib.MSX_ERR_INVALID, name


def test_the_wrappers_take_what_the_sampler_passes():
    sig = lambda f: list(inspect.signature(f).parameters)
    general = ['sidx', 'cidx', 'kind', 'p1', 'p2', 'g', 'fac', 'logu', 'swap_logu']
    G = _lib.Group
    assert sig(G.tempered_begin) == ['self', 'betas', 'counts', 'coords', 'll', 'lpr', 'max_chunk_steps']
    assert sig(G.tempered_enqueue) == ['self', 'slot'] + general
    assert sig(G.tempered_enqueue_drawn) == ['self', 'slot', 'nsteps', 'seeds', 'moves', 'first_iter']
    assert sig(G.tempered_collect) == ['self', 'slot', 'nsteps'] and sig(G.tempered_end) == ['self', 'want_state']
    assert sig(G.tempered_attach_series) == ['self', 'chain', 'dens', 'at_row'] and sig(G.tempered_adapt) == ['self', 'lag', 'time', 'k0']
    assert sig(G.tempered_betas) == ['self', 'slot', 'nsteps'] and sig(G.tempered_ladder) == ['self']
    assert sig(tempered.DeviceGroupTemperedSampler.__init__)[:4] == ['self', 'group', 'nwalkers', 'ndim']
    for name in ('ntemps', 'betas', 'beta_min', 'seeds', 'chunk', 'rng', 'moves', 'autocorr', 'adaptive', 'adaptation_lag', 'adaptation_time'):
        assert name in sig(tempered.DeviceGroupTemperedSampler.__init__), name
    for cls in (tempered.GroupTemperedSampler, tempered.DeviceGroupTemperedSampler):
        for name in ('run_mcmc', 'sample', 'reset', 'target', 'nwalkers'):
            assert hasattr(cls, name), (cls, name)
    for name in ('get_chain', 'get_log_like', 'get_betas', 'acceptance_fraction', 'swap_fraction', 'get_autocorr_time', 'get_summary',
                 'get_products', 'mean_log_like', 'log_evidence'):
        assert hasattr(tempered._TargetLadder, name) and getattr(tempered._TargetLadder, name) is getattr(tempered._Ladder, name), name


def test_the_kernels_sit_beside_the_single_target_ones():
    hip = open(os.path.join(CSRC, 'msx.hip')).read()
    assert hip.index('#include "tempered_kernels.h"') < hip.index('#include "group_tempered_kernels.h"') < hip.index('#include "group_kernel.h"')
    assert hip.index('#include "group_tempered_run.h"') > hip.index('int msx_series_evidence')
    src = open(os.path.join(CSRC, 'group_tempered_kernels.h')).read()
    for kernel in ('group_tempered_step_kernel', 'group_tempered_swap_kernel', 'group_tempered_swap_draw_kernel', 'group_tempered_adapt_kernel'):
        assert re.search(r'__global__ void __launch_bounds__\(\d+\)\s+' + kernel + r'\(', src), kernel
    # the swap draws are the single target's stream and stride, and the ladder step calls the shared inline pieces
    assert 'kSwapStream, p * kSwapStride + (unsigned int)w' in src
    for piece in ('ladder_kappa(', 'ladder_gap(', 'ladder_sums(', 'ladder_place(', 'ladder_valid('):
        assert piece in src, piece
    assert 'exp(' not in src.replace('ladder_exp(', '')                      # never a library's exp
    assert int(re.search(r'#define MSX_MAX_GROUP (\d+)', open(HDR).read()).group(1)) == tempered.MAX_TEMPS == 64


def test_design_md_holds_the_generated_table_and_the_bar_is_met():
    """DESIGN.md section 20's table is what tools/design_tables.py makes of profiles/group_tempered_bench.jsonl; the file holds
    the four shapes, and the 8 x 50 shapes meet the bar: one group run takes at most 0.5 of the targets' own ladders summed."""
    import json
    import sys
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    import design_tables as dt
    text = open(os.path.join(ROOT, 'DESIGN.md')).read()
    assert dt.GROUP_TEMPERED_BEGIN in text and dt.GROUP_TEMPERED_END in text
    block = text[text.index(dt.GROUP_TEMPERED_BEGIN) + len(dt.GROUP_TEMPERED_BEGIN):text.index(dt.GROUP_TEMPERED_END)]
    assert block.strip() == dt.build_group_tempered().strip() and block.strip()
    rows = [json.loads(ln) for ln in open(os.path.join(ROOT, 'profiles', 'group_tempered_bench.jsonl')) if ln.startswith('{')]
    shapes = {(r['targets'], r['ntemps'], r['walkers_per_rung']): r for r in rows}
    assert sorted(shapes) == [(1, 8, 256), (8, 4, 50), (8, 8, 50), (8, 8, 256)]
    for shape, r in shapes.items():
        assert len(r['group_rounds']) == len(r['solo_rounds']) == 5 and r['iters'] == 2048 and r['skip'] == 256
        assert r['target0_equals_its_solo_run'] and abs(r['ratio'] - r['group_us_per_iter'] / r['solo_sum_us_per_iter']) < 1e-12
        assert all(0.0 < x < 1.0 for x in r['swap_fraction_target0'])
        if shape[2] == 50:
            assert r['bar'] == 0.5 and r['meets_bar'] and r['ratio'] <= 0.5, (shape, r['ratio'])
