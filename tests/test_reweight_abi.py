"""CPU: the five reweighting calls (include/msx.h) are declared, exported and mirrored with the right
ctypes signatures; null series are refused without a device; the tile constant is the header's; the kernels
(csrc/reweight_kernels.h) compile alone for gfx950 with no scratch, no floating-point atomics and no assembly.  No compute
calls (no GPU here)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import common  # noqa: F401
from mcmc_spec_amd import _lib, reweight

ROOT = common.ROOT
HDR = os.path.join(ROOT, 'include', 'msx.h')
CSRC = os.path.join(ROOT, 'mcmc_spec_amd', 'csrc')
DP, UP, VP, IP, I32P = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)
SEL = ['int64_t n', 'int64_t discard', 'int64_t thin']
PARAMS = {
    'msx_series_logprob': ['msx_series *src', 'msx_ctx **ctxs', 'int32_t mode', 'int64_t row0', 'int64_t nrows', 'msx_series *dst',
                           'int32_t *worst_status'],
    'msx_series_lincomb': ['int32_t nsrc', 'msx_series **srcs', 'const int32_t *cols', 'const double *coef', 'int64_t row0', 'int64_t nrows',
                           'msx_series *dst'],
    'msx_series_weights': ['msx_series *logw'] + SEL + ['msx_series *w_dst', 'double *stats'],
    'msx_series_wmoments': ['msx_series *src', 'msx_series *w'] + SEL + ['const uint32_t *cols', 'int32_t ncols', 'double *sumw',
                                                                         'double *mean', 'double *cov'],
    'msx_series_resample': ['msx_series *src', 'msx_series *w'] + SEL + ['uint64_t seed', 'const int64_t *nout', 'msx_series **dst',
                                                                         'int64_t *index_out'],
}
SEL_T = [C.c_int64, C.c_int64, C.c_int64]
ARGTYPES = {
    'msx_series_logprob': [VP, C.POINTER(VP), C.c_int32, C.c_int64, C.c_int64, VP, I32P],
    'msx_series_lincomb': [C.c_int32, C.POINTER(VP), I32P, DP, C.c_int64, C.c_int64, VP],
    'msx_series_weights': [VP] + SEL_T + [VP, DP],
    'msx_series_wmoments': [VP, VP] + SEL_T + [UP, C.c_int32, DP, DP, DP],
    'msx_series_resample': [VP, VP] + SEL_T + [C.c_uint64, IP, C.POINTER(VP), IP],
}
KERNELS = {'rw_gather_theta_kernel', 'rw_put_logp_kernel', 'rw_lincomb_kernel', 'rw_max_kernel', 'rw_exp_kernel', 'rw_stat_kernel',
           'rw_stat_combine_kernel', 'rw_wsum_kernel', 'rw_wmean_kernel', 'rw_wcross_kernel', 'rw_wcov_kernel', 'rw_scan_local_kernel',
           'rw_scan_tiles_kernel', 'rw_scan_add_kernel', 'rw_draw_kernel'}


def test_the_functions_are_declared_exported_and_mirrored():
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load()
    txt = re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)
    for name in PARAMS:
        m = re.search(r'\bint ' + name + r'\s*\(([^)]*)\)\s*;', txt)
        assert m, name
        assert [' '.join(p.split()) for p in m.group(1).split(',')] == PARAMS[name]
        assert name in _lib.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == ARGTYPES[name]
        assert txt.index('typedef struct msx_series msx_series;') < txt.index(name)
    assert len(set(_lib.EXPORTED)) == len(_lib.EXPORTED)
    tile = int(re.search(r'#define MSX_RESAMPLE_TILE (\d+)', txt).group(1))
    assert tile == _lib.RESAMPLE_TILE == reweight.TILE and tile % reweight.LANES == 0
    hip = open(os.path.join(CSRC, 'msx.hip')).read()
    assert hip.index('#include "mode_kernels.h"') < hip.index('#include "reweight_kernels.h"')
    text = open(os.path.join(CSRC, 'reweight_kernels.h')).read()
    assert 'kRwTile = MSX_RESAMPLE_TILE' in text and int(re.search(r'kRwThreads = (\d+)', text).group(1)) == reweight.LANES
    assert int(re.search(r'kRwStream = (\d+)', text).group(1)) == reweight.STREAM
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(_lib.Series.logprob) == ['self', 'contexts', 'dst', 'mode', 'row0', 'nrows']
    assert sig(_lib.Series.lincomb) == ['terms', 'dst', 'row0', 'nrows'] and isinstance(_lib.Series.__dict__['lincomb'], staticmethod)
    assert sig(_lib.Series.weights) == ['self', 'n', 'w_dst', 'discard', 'thin']
    assert sig(_lib.Series.wmoments) == ['self', 'w', 'n', 'discard', 'thin', 'cols', 'cov']
    assert sig(_lib.Series.resample) == ['self', 'w', 'n', 'nout', 'dst', 'discard', 'thin', 'seed']
    assert sig(reweight.rescore) == ['series', 'n', 'engines', 'mode'] and sig(reweight.log_weights)[0] == 'terms'
    from mcmc_spec_amd import group, sampler, tempered
    for cls in (sampler.DeviceEnsembleSampler, group.DeviceGroupSampler):
        assert sig(cls.get_reweighted) == ['self', 'engines_new', 'mode', 'discard', 'thin']
    assert sig(tempered.DeviceTemperedSampler.get_reweighted) == ['self', 'engines_new', 't', 'mode', 'discard', 'thin']
    assert tempered._TargetLadder.get_reweighted is tempered._Ladder.get_reweighted


def test_null_series_are_refused_without_a_device():
    lib = _lib.load()
    d = (C.c_double * 64)()
    i64 = (C.c_int64 * 4)()
    assert lib.msx_series_logprob(None, None, _lib.MODE_LOGPOST, 0, 1, None, None) == _lib.MSX_ERR_INVALID
    assert lib.msx_series_lincomb(1, None, None, d, 0, 1, None) == _lib.MSX_ERR_INVALID
    assert lib.msx_series_weights(None, 1, 0, 1, None, d) == _lib.MSX_ERR_INVALID
    assert lib.msx_series_wmoments(None, None, 1, 0, 1, None, 1, d, d, d) == _lib.MSX_ERR_INVALID
    assert lib.msx_series_resample(None, None, 1, 0, 1, 0, i64, None, None) == _lib.MSX_ERR_INVALID


def test_the_kernels_compile_alone_for_gfx950_without_scratch_or_float_atomics():
    text = open(os.path.join(CSRC, 'reweight_kernels.h')).read()
    code = re.sub(r'//.*', '', text)
    # the one atomic is the integer maximum of the sample statuses; nothing floating-point goes through an atomic
    assert code.count('atomic') == 1 and 'atomicMax(worst, st)' in code and 'asm' not in code
    assert set(re.findall(r'\b(rw_\w+_kernel)\(', code)) == KERNELS
    # every kernel that does arithmetic on doubles keeps the compiler from contracting a * b + c
    for name in KERNELS - {'rw_gather_theta_kernel', 'rw_put_logp_kernel', 'rw_max_kernel'}:
        body = code[code.index(name + '('):]
        assert body[body.index('{'):].lstrip('{\n ').startswith('#pragma clang fp contract(off)'), name
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, 'rk.hip')
        with open(src, 'w') as f:
            f.write('#include <hip/hip_runtime.h>\n#include <stdint.h>\n#include <math.h>\n#define MSX_MAX_DIM 8\n#define MSX_W_REJECT 1\n'
                    '#define MSX_RESAMPLE_TILE {}\n#include "{}"\n'.format(_lib.RESAMPLE_TILE, os.path.join(CSRC, 'reweight_kernels.h')))
        out = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                              '-Rpass-analysis=kernel-resource-usage', '-o', os.path.join(d, 'rk.s'), src],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        asm = open(os.path.join(d, 'rk.s')).read()
    lines = out.stderr.splitlines()
    assert not [ln for ln in lines if 'reweight_kernels.h' in ln and 'warning:' in ln]
    seen = set()
    for i, ln in enumerate(lines):
        m = re.search(r'Function Name: _Z\d+(rw_\w+?_kernel)', ln)
        if m:
            block = '\n'.join(lines[i:i + 14])
            s = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block)
            assert s and int(s.group(1)) == 0, block
            seen.add(m.group(1))
    assert seen == KERNELS, seen
    assert 'scratch_' not in asm
    assert not re.search(r'atomic_(add|min|max|pk_add)_f(32|64)', asm)
    # no a * b + c was contracted: fused multiply-adds appear only where the source divides (the correctly rounded quotient's
    # sequence) or calls the library's exp
    bodies = dict(re.findall(r'^_Z\d+(rw_\w+?_kernel)\w*:[^\n]*\n(.*?)\.Lfunc_end', asm, flags=re.S | re.M))
    assert set(bodies) == KERNELS
    fused = {name for name, body in bodies.items() if re.search(r'v_fmac?_f64', body)}
    assert fused == {'rw_exp_kernel', 'rw_stat_combine_kernel', 'rw_wmean_kernel', 'rw_wcov_kernel'}, fused
    for name in fused - {'rw_exp_kernel'}:
        assert 'v_div_fixup_f64' in bodies[name], name
