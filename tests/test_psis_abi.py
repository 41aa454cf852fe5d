"""CPU: msx_series_psis (include/msx.h) is declared, exported and mirrored with the right ctypes
signature; the header's constants are _lib's and the definition's; a null series is refused without a device; the kernels
(csrc/psis_kernels.h) compile for gfx950 with no scratch and no floating-point atomics, within the LDS the header states.  No
compute calls (no GPU here)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import numpy as np

import common  # noqa: F401
from mcmc_spec_amd import _lib, psis, reweight

ROOT = common.ROOT
HDR = os.path.join(ROOT, 'include', 'msx.h')
CSRC = os.path.join(ROOT, 'mcmc_spec_amd', 'csrc')
DP, VP, IP, I32P = C.POINTER(C.c_double), C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int32)
PARAMS = ['msx_series *logw', 'int64_t n', 'int64_t discard', 'int64_t thin', 'const int64_t *tail_len', 'msx_series *w_dst',
          'msx_series *lw_dst', 'double *khat', 'int32_t *status', 'int64_t *tail_count', 'double *stats', 'int64_t *tail_index']
ARGTYPES = [VP, C.c_int64, C.c_int64, C.c_int64, IP, VP, VP, DP, I32P, IP, DP, IP]
POINTWISE = {
    'msx_pointwise_nobs': (['msx_ctx *ctx', 'int64_t *npix', 'int32_t *n_contrast', 'int32_t *n_phot'], [VP, IP, I32P, I32P]),
    'msx_predictive_pointwise': (['msx_ctx *ctx', 'const double *theta', 'int64_t n', 'int32_t ndim', 'double reff', 'int64_t scratch_bytes',
                                  'double *out', 'int32_t *status', 'int64_t *count', 'int64_t *tail_len', 'double *ll_out'],
                                 [VP, DP, C.c_int64, C.c_int32, C.c_double, C.c_int64, DP, I32P, IP, IP, DP]),
    'msx_series_pointwise': (['msx_series *src', 'msx_ctx **ctxs', 'int64_t n', 'int64_t discard', 'int64_t thin', 'double reff',
                              'int64_t scratch_bytes', 'double *out', 'int64_t *count', 'int64_t *tail_len', 'int32_t *worst_status',
                              'double *ll_out'],
                             [VP, C.POINTER(VP), C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_int64, DP, IP, IP, I32P, DP]),
}
KERNELS = {'psis_scan_kernel', 'psis_fill_kernel', 'psis_reduce_kernel'}


def header():
    return re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)


def test_the_function_is_declared_exported_and_mirrored():
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load()
    txt = header()
    sig = lambda f: list(inspect.signature(f).parameters)
    m = re.search(r'\bint msx_series_psis\s*\(([^)]*)\)\s*;', txt)
    assert m and [' '.join(p.split()) for p in m.group(1).split(',')] == PARAMS
    assert 'msx_series_psis' in _lib.EXPORTED and len(set(_lib.EXPORTED)) == len(_lib.EXPORTED)
    fn = lib.msx_series_psis
    assert fn.restype is C.c_int and list(fn.argtypes) == ARGTYPES and len(ARGTYPES) == len(PARAMS)
    for name, (params, argtypes) in POINTWISE.items():
        m = re.search(r'\bint ' + name + r'\s*\(([^)]*)\)\s*;', txt)
        assert m and [' '.join(p.split()) for p in m.group(1).split(',')] == params, name
        assert name in _lib.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
    hip = open(os.path.join(CSRC, 'msx.hip')).read()
    assert hip.index('#include "reweight_kernels.h"') < hip.index('#include "psis_kernels.h"') < hip.index('#include "pointwise_kernels.h"')
    assert hip.index('#include "predictive_kernels.h"') < hip.index('#include "pointwise_kernels.h"')
    # the new kernels' names stay clear of the patterns that count the predictive and the products kernels
    pw = open(os.path.join(CSRC, 'pointwise_kernels.h')).read()
    names = set(re.findall(r'\b(\w+_kernel)\(const Pw', pw))
    assert names == {'pointwise_pixel_kernel', 'pointwise_band_kernel', 'pointwise_reduce_kernel'}
    assert not any(re.search(r'predictive_(sample|fill|reduce)_kernel|products_kernel|products_spectra_kernel|composite_parts_kernel', n) for n in names)
    assert sig(_lib.Context.predictive_pointwise) == ['self', 'theta', 'reff', 'scratch_bytes', 'want_matrix']
    assert sig(_lib.Series.pointwise) == ['self', 'contexts', 'n', 'discard', 'thin', 'reff', 'scratch_bytes', 'want_matrix']
    assert sig(psis.loo) == ['engine', 'theta', 'reff', 'pointwise', 'scratch_mb', 'wl']
    assert sig(psis.loo_series) == ['series', 'n', 'engines', 'discard', 'thin', 'reff', 'pointwise', 'scratch_mb', 'wl']
    from mcmc_spec_amd import group, sampler, tempered
    assert sig(sampler.DeviceEnsembleSampler.get_loo) == ['self', 'discard', 'thin', 'reff']
    assert sig(group.DeviceGroupSampler.get_loo) == ['self', 'discard', 'thin', 'reff', 'k']
    assert sig(tempered.DeviceTemperedSampler.get_loo) == ['self', 't', 'discard', 'thin', 'reff']
    assert sig(_lib.Series.psis) == ['self', 'n', 'tail_len', 'w_dst', 'lw_dst', 'discard', 'thin', 'want_tail']
    assert sig(psis.smooth_series) == ['logw', 'n', 'w_dst', 'discard', 'thin', 'reff', 'lw_dst', 'want_tail']
    assert sig(psis.smooth) == ['lr', 'tail_len'] and sig(psis.tail_len) == ['S', 'reff']
    assert sig(reweight.Reweighted.smooth) == ['self', 'reff'] and issubclass(psis.Smoothed, reweight.Reweighted)


def test_the_headers_constants_are_the_bindings():
    txt = header()
    num = lambda name: re.search(r'#define ' + name + r' \(?(-?[\d.]+)\)?', txt).group(1)
    assert int(num('MSX_POINTWISE_MATRIX_MAX')) == _lib.POINTWISE_MATRIX_MAX == 1 << 30
    assert int(num('MSX_PSIS_TAIL_MAX')) == _lib.PSIS_TAIL_MAX == psis.TAIL_MAX == 4096
    assert int(num('MSX_PSIS_MIN_TAIL')) == _lib.PSIS_MIN_TAIL == psis.MIN_TAIL == 5
    assert int(num('MSX_PSIS_OK')) == _lib.PSIS_OK == psis.OK and int(num('MSX_PSIS_SHORT_TAIL')) == _lib.PSIS_SHORT_TAIL == psis.SHORT_TAIL
    assert float(num('MSX_PSIS_LOG_TINY')) == _lib.PSIS_LOG_TINY == psis.LOG_TINY == float(np.log(np.finfo(np.float64).tiny))
    text = open(os.path.join(CSRC, 'psis_kernels.h')).read()
    assert 'kPsTailMax = MSX_PSIS_TAIL_MAX' in text and int(re.search(r'kPsThreads = (\d+)', text).group(1)) == reweight.LANES
    # m = 30 + floor(sqrt(n)) fit points fit the tables
    assert 30 + int(np.floor(np.sqrt(_lib.PSIS_TAIL_MAX))) <= int(re.search(r'kPsFitMax = (\d+)', text).group(1))
    # the largest tail the papers' expression asks for at the sizes DESIGN.md names
    assert psis.tail_len(750000) <= psis.TAIL_MAX and psis.tail_len(1800000) <= psis.TAIL_MAX


def test_a_null_series_is_refused_without_a_device():
    lib = _lib.load()
    d = (C.c_double * 16)()
    i64 = (C.c_int64 * 4)()
    i32 = (C.c_int32 * 4)()
    assert lib.msx_series_psis(None, 1, 0, 1, i64, None, None, d, i32, i64, d, None) == _lib.MSX_ERR_INVALID
    assert lib.msx_pointwise_nobs(None, i64, i32, i32) == _lib.MSX_ERR_INVALID
    assert lib.msx_predictive_pointwise(None, d, 1, 6, 1.0, 0, d, i32, i64, i64, None) == _lib.MSX_ERR_INVALID
    assert lib.msx_series_pointwise(None, None, 1, 0, 1, 1.0, 0, d, i64, i64, i32, None) == _lib.MSX_ERR_INVALID


def test_the_kernels_compile_for_gfx950_without_scratch_or_float_atomics():
    text = open(os.path.join(CSRC, 'psis_kernels.h')).read()
    code = re.sub(r'//.*', '', text)
    # two atomics, both on integers: the count of bad values and the tail's slot counter in LDS
    assert code.count('atomic') == 2 and 'atomicAdd(&cnt, 1u)' in code and '(unsigned long long)rc[0]' in code and 'asm' not in code
    assert set(re.findall(r'\b(psis_\w+_kernel)\(', code)) == KERNELS
    body = code[code.index('psis_reduce_kernel('):]
    assert body[body.index('{'):].lstrip('{\n ').startswith('#pragma clang fp contract(off)')
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, 'pk.hip')
        with open(src, 'w') as f:
            f.write('#include <hip/hip_runtime.h>\n#include <stdint.h>\n#include <math.h>\n#include "{}"\n#include "{}"\n#include "{}"\n'.format(
                HDR, os.path.join(CSRC, 'reweight_kernels.h'), os.path.join(CSRC, 'psis_kernels.h')))
        out = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-c', '--cuda-device-only',
                              '-Rpass-analysis=kernel-resource-usage', '-o', os.path.join(d, 'pk.o'), src],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    assert not [ln for ln in lines if 'psis_kernels.h' in ln and 'warning:' in ln]
    seen = {}
    for i, ln in enumerate(lines):
        m = re.search(r'Function Name: _Z\d+(psis_\w+?_kernel)', ln)
        if m:
            block = '\n'.join(lines[i:i + 14])
            s = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block)
            lds = re.search(r'LDS Size \[bytes/block\]: (\d+)', block)
            assert s and int(s.group(1)) == 0, block
            seen[m.group(1)] = int(lds.group(1))
    assert set(seen) == KERNELS, seen
    # values (8 B) and indices (4 B) of the tail, and at most 5 KB more: three workgroups fit a CU's 160 KiB
    assert 12 * _lib.PSIS_TAIL_MAX <= seen['psis_reduce_kernel'] <= 12 * _lib.PSIS_TAIL_MAX + 5 * 1024
