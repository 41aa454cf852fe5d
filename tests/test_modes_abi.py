"""CPU: msx_series_modes and msx_series_mode_labels (include/msx.h) are declared, exported and mirrored
with the right ctypes signatures; a null series is refused without a device; the kernels (csrc/mode_kernels.h) compile alone
for gfx950 with no scratch, no atomics and no assembly.  No compute calls (no GPU here)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import common  # noqa: F401
from mcmc_spec_amd import _lib, modes

ROOT = common.ROOT
HDR = os.path.join(ROOT, 'include', 'msx.h')
CSRC = os.path.join(ROOT, 'mcmc_spec_amd', 'csrc')
DP, UP, VP, IP = C.POINTER(C.c_double), C.POINTER(C.c_uint32), C.c_void_p, C.POINTER(C.c_int64)
I32P, U8P = C.POINTER(C.c_int32), C.POINTER(C.c_uint8)
SEL = ['msx_series *s', 'int64_t n', 'int64_t discard', 'int64_t thin', 'const uint32_t *cols', 'int32_t ncols', 'const double *center',
       'const double *scale', 'int32_t ncomp']
PARAMS = {
    'msx_series_modes': SEL + ['int32_t nstarts', 'const int32_t *split_col', 'const double *split_at', 'int32_t max_iter', 'double tol',
                               'double ridge', 'double *weight', 'double *mean', 'double *cov', 'double *loglik', 'int32_t *niter',
                               'int32_t *status', 'int64_t *nbad'],
    'msx_series_mode_labels': SEL + ['const double *weight', 'const double *mean', 'const double *cov', 'uint8_t *labels_out',
                                     'int64_t *counts_out', 'msx_series **dst'],
}
SEL_T = [VP, C.c_int64, C.c_int64, C.c_int64, UP, C.c_int32, DP, DP, C.c_int32]
ARGTYPES = {
    'msx_series_modes': SEL_T + [C.c_int32, I32P, DP, C.c_int32, C.c_double, C.c_double, DP, DP, DP, DP, I32P, I32P, IP],
    'msx_series_mode_labels': SEL_T + [DP, DP, DP, U8P, IP, C.POINTER(VP)],
}


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
    assert int(re.search(r'#define MSX_MODES_MAX (\d+)', txt).group(1)) == _lib.MODES_MAX == modes.MODES_MAX == 4
    assert int(re.search(r'#define MSX_MAX_DIM (\d+)', txt).group(1)) == modes.MAX_DIM
    for name, value in (('CONVERGED', modes.CONVERGED), ('MAXITER', modes.MAXITER), ('COLLAPSED', modes.COLLAPSED)):
        assert int(re.search(r'#define MSX_MODES_' + name + r' (\d+)', txt).group(1)) == value
    hip = open(os.path.join(CSRC, 'msx.hip')).read()
    assert hip.index('#include "predictive_kernels.h"') < hip.index('#include "mode_kernels.h"')
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(_lib.Series.modes) == ['self', 'n', 'discard', 'thin', 'cols', 'center', 'scale', 'ncomp', 'split_col', 'split_at', 'max_iter',
                                      'tol', 'ridge']
    assert sig(_lib.Series.mode_labels) == ['self', 'n', 'discard', 'thin', 'cols', 'center', 'scale', 'weight', 'mean', 'cov', 'dst',
                                            'want_labels']
    assert sig(modes.fit)[:9] == ['chain', 'counts', 'cols', 'ncomp', 'max_iter', 'tol', 'ridge', 'discard', 'thin']
    p = inspect.signature(modes.fit).parameters
    assert [p[n].default for n in sig(modes.fit)[1:9]] == [None, None, 2, 50, 1e-10, 1e-6, 0, 1]


def test_a_null_series_is_refused_without_a_device():
    lib = _lib.load()
    d = (C.c_double * 64)()
    i32 = (C.c_int32 * 4)()
    i64 = (C.c_int64 * 4)()
    assert lib.msx_series_modes(None, 8, 0, 1, None, 1, d, d, 2, 1, i32, d, 50, 1e-10, 1e-6, d, d, d, d, i32, i32, i64) == _lib.MSX_ERR_INVALID
    assert lib.msx_series_mode_labels(None, 8, 0, 1, None, 1, d, d, 2, d, d, d, None, i64, None) == _lib.MSX_ERR_INVALID


def test_the_kernels_compile_alone_for_gfx950_without_scratch_or_atomics():
    text = open(os.path.join(CSRC, 'mode_kernels.h')).read()
    code = re.sub(r'//.*', '', text)
    assert 'atomic' not in code and 'asm' not in code
    # the five kernels, the tree and the E-step they share
    assert code.count('__global__ void __launch_bounds__') == 5 and code.count('#pragma clang fp contract(off)') == 7
    for m in re.finditer(r'__global__ void __launch_bounds__[^{]*\{\n(.*)\n', code):
        assert m.group(1).strip() == '#pragma clang fp contract(off)', m.group(0)[:80]
    assert int(re.search(r'kModeThreads = (\d+)', text).group(1)) == 256 and int(re.search(r'kModeTile = (\d+)', text).group(1)) == 4096
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, 'mk.hip')
        with open(src, 'w') as f:
            f.write('#include <hip/hip_runtime.h>\n#include <stdint.h>\n#include <math.h>\n#define MSX_MAX_DIM 8\n#define MSX_MODES_MAX 4\n'
                    '#include "{}"\n'.format(os.path.join(CSRC, 'mode_kernels.h')))
        out = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                              '-Rpass-analysis=kernel-resource-usage', '-o', os.path.join(d, 'mk.s'), src],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    assert not [ln for ln in lines if 'mode_kernels.h' in ln and 'warning:' in ln]
    seen = {}
    for i, ln in enumerate(lines):
        m = re.search(r'Function Name: _Z\d+(mode_\w+?_kernel)(ILi(\d)E)?', ln)
        if m:
            block = '\n'.join(lines[i:i + 14])
            s = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block)
            assert s and int(s.group(1)) == 0, block
            seen.setdefault(m.group(1), set()).add(int(m.group(3) or 0))
    every = set(range(1, 9))
    assert seen == {'mode_stats_kernel': every, 'mode_label_kernel': every, 'mode_mstep_kernel': {0}, 'mode_scan_kernel': {0},
                    'mode_scatter_kernel': {0}}, seen
