"""CPU: msx_series_moments (include/msx.h) is declared, exported and mirrored with the right ctypes
signature; the kernels (csrc/diag_kernels.h) compile for gfx950 with no scratch and no atomics; a null series is refused
without a device; every sampler class has get_rhat and get_moments.  No compute calls (no GPU here)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import common  # noqa: F401
from mcmc_spec_amd import _lib, group, sampler, tempered

ROOT = common.ROOT
HDR = os.path.join(ROOT, 'include', 'msx.h')
CSRC = os.path.join(ROOT, 'mcmc_spec_amd', 'csrc')
DP, UP, VP = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_void_p
PARAMS = ['msx_series *s', 'int64_t n', 'int64_t discard', 'int64_t thin', 'const uint32_t *cols', 'int32_t ncols', 'double *within',
          'double *var_plus', 'double *between', 'double *mean', 'double *cov']
ARGTYPES = [VP, C.c_int64, C.c_int64, C.c_int64, UP, C.c_int32, DP, DP, DP, DP, DP]


def test_the_function_is_declared_exported_and_mirrored():
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load()
    txt = re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)
    m = re.search(r'\bint msx_series_moments\s*\(([^)]*)\)\s*;', txt)
    assert m
    assert [' '.join(p.split()) for p in m.group(1).split(',')] == PARAMS
    assert 'msx_series_moments' in _lib.EXPORTED and len(set(_lib.EXPORTED)) == len(_lib.EXPORTED)
    fn = lib.msx_series_moments
    assert fn.restype is C.c_int and list(fn.argtypes) == ARGTYPES
    assert txt.index('typedef struct msx_series msx_series;') < txt.index('msx_series_moments')
    hip = open(os.path.join(CSRC, 'msx.hip')).read()
    assert hip.index('#include "evidence_kernels.h"') < hip.index('#include "diag_kernels.h"')


def test_a_null_series_is_refused_without_a_device():
    lib = _lib.load()
    out = (C.c_double * 4)()
    assert lib.msx_series_moments(None, 8, 0, 1, None, 1, out, out, out, out, None) == _lib.MSX_ERR_INVALID


def test_the_kernels_compile_for_gfx950_without_scratch_or_atomics():
    text = open(os.path.join(CSRC, 'diag_kernels.h')).read()
    code = re.sub(r'//.*', '', text)
    assert 'atomic' not in code and 'asm' not in code
    assert code.count('#pragma clang fp contract(off)') == 6          # the five kernels and the tree they share
    assert int(re.search(r'kDiagThreads = (\d+)', text).group(1)) == 256
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, 'dg.hip')
        with open(src, 'w') as f:
            f.write('#include <hip/hip_runtime.h>\n#include <stdint.h>\n#include <math.h>\n#define MSX_MAX_DIM 8\n#include "{}"\n'.format(
                os.path.join(CSRC, 'diag_kernels.h')))
        out = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                              '-Rpass-analysis=kernel-resource-usage', '-o', os.path.join(d, 'dg.s'), src],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    assert not [ln for ln in lines if 'diag_kernels.h' in ln and 'warning:' in ln]
    seen = set()
    for i, ln in enumerate(lines):
        m = re.search(r'Function Name: _Z\d+(\w+?_kernel)', ln)
        if m:
            block = '\n'.join(lines[i:i + 14])
            s = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block)
            assert s and int(s.group(1)) == 0, block
            seen.add(m.group(1))
    assert seen == {'diag_sum_kernel', 'diag_mean_kernel', 'diag_dev_kernel', 'diag_cross_kernel', 'diag_combine_kernel'}, seen


def test_every_sampler_has_get_rhat_and_get_moments():
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(_lib.Series.moments) == ['self', 'n', 'discard', 'thin', 'cols', 'cov']
    d = inspect.signature(_lib.Series.moments).parameters
    assert (d['discard'].default, d['thin'].default, d['cols'].default, d['cov'].default) == (0, 1, None, True)
    for cls, lead, default in ((sampler.EnsembleSampler, [], None), (sampler.DeviceEnsembleSampler, [], None),
                               (group.GroupSampler, ['k'], None), (group.DeviceGroupSampler, ['k'], None),
                               (tempered.TemperedSampler, ['t'], 0), (tempered.DeviceTemperedSampler, ['t'], 0),
                               (tempered._TargetLadder, ['t'], 0)):
        for name in ('get_rhat', 'get_moments'):
            fn = getattr(cls, name)
            assert sig(fn) == ['self'] + lead + ['discard', 'thin', 'cols'], (cls, name)
            p = inspect.signature(fn).parameters
            assert (p['discard'].default, p['thin'].default, p['cols'].default) == (0, 1, None)
            if lead:
                assert p[lead[0]].default == default
    for fn in (sampler.run_reference_protocol, group.run_group_protocol):
        assert inspect.signature(fn).parameters['rhat'].default is None
