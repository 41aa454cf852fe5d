"""CPU: the tempering ABI (include/msx.h, msx_tempered_*): the six functions are declared, exported and mirrored with the
right ctypes signatures, the wrappers take what the samplers pass, the constants mirror each other.  No compute calls (no GPU here)."""
import ctypes as C
import inspect
import os
import re

import common  # noqa: F401
from mcmc_spec_amd import _lib, moves, tempered

ROOT = common.ROOT
HDR = os.path.join(ROOT, 'include', 'msx.h')

I32P, DP, I64P, U64P, VP = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.c_void_p
SETP = C.POINTER(moves.MsxMoveSet)
GENERAL = ['const int32_t *sidx', 'const int32_t *cidx', 'const int32_t *kind', 'const int32_t *p1', 'const int32_t *p2',
           'const double *g', 'const double *fac', 'const double *logu', 'const double *swap_logu']
FUNCTIONS = {
    'msx_tempered_begin': (['msx_ctx *ctx', 'int32_t ntemps', 'const double *betas', 'int64_t nw', 'int32_t ndim', 'int64_t max_chunk_steps',
                            'const double *coords', 'const double *ll', 'const double *lpr'],
                           [VP, C.c_int32, DP, C.c_int64, C.c_int32, C.c_int64, DP, DP, DP]),
    'msx_tempered_enqueue': (['msx_ctx *ctx', 'int32_t slot', 'int64_t nsteps'] + GENERAL, [VP, C.c_int32, C.c_int64] + [I32P] * 5 + [DP] * 4),
    'msx_tempered_enqueue_drawn': (['msx_ctx *ctx', 'int32_t slot', 'int64_t nsteps', 'const uint64_t *seeds', 'const msx_move_set *set',
                                    'int64_t first_iter'], [VP, C.c_int32, C.c_int64, U64P, SETP, C.c_int64]),
    'msx_tempered_draw': (['msx_ctx *ctx', 'int32_t ntemps', 'const uint64_t *seeds', 'const msx_move_set *set', 'int64_t first_iter',
                           'int64_t nsteps', 'int64_t nw', 'int32_t ndim'] + [p.replace('const ', '') for p in GENERAL],
                          [VP, C.c_int32, U64P, SETP, C.c_int64, C.c_int64, C.c_int64, C.c_int32] + [I32P] * 5 + [DP] * 4),
    'msx_tempered_collect': (['msx_ctx *ctx', 'int32_t slot', 'double *chain', 'double *ll_chain', 'double *lpr_chain', 'int64_t *naccept',
                              'int64_t *nswap', 'int32_t *worst'], [VP, C.c_int32, DP, DP, DP, I64P, I64P, I32P]),
    'msx_tempered_end': (['msx_ctx *ctx', 'double *coords', 'double *ll', 'double *lpr'], [VP, DP, DP, DP]),
}


def header():
    return re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)


def test_the_six_functions_are_declared_exported_and_mirrored():
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
    assert sorted(n for n in _lib.EXPORTED if n.startswith('msx_tempered_')) == sorted(FUNCTIONS)
    assert sorted(set(re.findall(r'\b(msx_tempered_[a-z_]+)\s*\(', txt))) == sorted(FUNCTIONS)


def test_the_wrappers_take_what_the_samplers_pass():
    sig = lambda f: list(inspect.signature(f).parameters)
    general = ['sidx', 'cidx', 'kind', 'p1', 'p2', 'g', 'fac', 'logu', 'swap_logu']
    assert sig(_lib.Context.tempered_begin) == ['self', 'betas', 'coords', 'll', 'lpr', 'max_chunk_steps']
    assert sig(_lib.Context.tempered_enqueue) == ['self', 'slot'] + general
    assert sig(_lib.Context.tempered_enqueue_drawn) == ['self', 'slot', 'nsteps', 'seeds', 'moves', 'first_iter']
    assert sig(_lib.Context.tempered_draw) == ['self', 'seeds', 'moves', 'first_iter', 'nsteps', 'nw', 'ndim']
    assert sig(_lib.Context.tempered_collect) == ['self', 'slot', 'nsteps'] and sig(_lib.Context.tempered_end) == ['self', 'want_state']
    from mcmc_spec_amd import mft6
    assert 'betas' in inspect.signature(mft6.device_sampler).parameters
    for cls in (tempered.TemperedSampler, tempered.DeviceTemperedSampler):
        for name in ('run_mcmc', 'sample', 'reset', 'get_chain', 'get_log_like', 'get_log_prior', 'get_log_prob', 'acceptance_fraction',
                     'swap_fraction', 'get_last_sample'):
            assert hasattr(cls, name), (cls, name)
        assert sig(cls.get_chain) == ['self', 't', 'flat', 'thin', 'discard']


def test_the_constants_mirror_each_other():
    txt = open(HDR).read()
    assert int(re.search(r'#define MSX_MAX_GROUP (\d+)', txt).group(1)) == tempered.MAX_TEMPS == _lib.MAX_GROUP == 64
    assert int(re.search(r'#define MSX_W_REJECT (\d+)', txt).group(1)) == tempered.W_REJECT == _lib.W_REJECT
    src = open(os.path.join(ROOT, 'mcmc_spec_amd', 'csrc', 'tempered_kernels.h')).read()
    assert int(re.search(r'kSwapStream = (\d+)u', src).group(1)) == tempered.SWAP_STREAM == 14
    assert int(re.search(r'kSwapStride = (\d+)u', src).group(1)) == tempered.SWAP_STRIDE == 4096
    assert 63 * tempered.SWAP_STRIDE + 4095 < 1 << 24
    hip = open(os.path.join(ROOT, 'mcmc_spec_amd', 'csrc', 'msx.hip')).read()
    assert hip.index('#include "move_kernels.h"') < hip.index('#include "tempered_kernels.h"')
