"""CPU: the ladder's device series and the evidence reduction (include/msx.h, msx_series_attach_tempered,
msx_series_evidence) are declared, exported and mirrored with the right ctypes signatures; the
evidence kernels (csrc/evidence_kernels.h) compile for gfx950 with no scratch and no atomics; the Python layer takes what
the issue names; what can be refused without a device is refused.  No compute calls (no GPU here)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import pytest

import common  # noqa: F401
from mcmc_spec_amd import _lib, tempered

ROOT = common.ROOT
HDR = os.path.join(ROOT, 'include', 'msx.h')
CSRC = os.path.join(ROOT, 'mcmc_spec_amd', 'csrc')
DP, VP = C.POINTER(C.c_double), C.c_void_p
FUNCTIONS = {
    'msx_series_attach_tempered': (['msx_ctx *ctx', 'msx_series *chain', 'msx_series *dens', 'int64_t at_row'], [VP, VP, VP, C.c_int64]),
    'msx_series_evidence': (['msx_series *s', 'int64_t n', 'int64_t discard', 'int64_t thin', 'int32_t col', 'const double *db',
                             'int32_t nblocks', 'double *mean_out', 'double *lme_out'],
                            [VP, C.c_int64, C.c_int64, C.c_int64, C.c_int32, DP, C.c_int32, DP, DP]),
}


def test_the_two_functions_are_declared_exported_and_mirrored():
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load()
    txt = re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)
    for name, (params, argtypes) in FUNCTIONS.items():
        m = re.search(r'\bint ' + name + r'\s*\(([^)]*)\)\s*;', txt)
        assert m, name
        assert [' '.join(p.split()) for p in m.group(1).split(',')] == params, name
        assert name in _lib.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name
    assert txt.index('typedef struct msx_series msx_series;') < txt.index('msx_series_attach_tempered')   # (a C header: declared before use)
    hip = open(os.path.join(CSRC, 'msx.hip')).read()
    assert hip.index('#include "summary_kernels.h"') < hip.index('#include "evidence_kernels.h"')


def test_null_handles_are_refused_without_a_device():
    lib = _lib.load()
    out = (C.c_double * 4)()
    assert lib.msx_series_attach_tempered(None, None, None, 0) == _lib.MSX_ERR_INVALID
    assert lib.msx_series_evidence(None, 1, 0, 1, 0, None, 1, out, None) == _lib.MSX_ERR_INVALID


def test_evidence_kernels_compile_for_gfx950_without_scratch_or_atomics():
    text = open(os.path.join(CSRC, 'evidence_kernels.h')).read()
    code = re.sub(r'//.*', '', text)
    assert 'atomic' not in code and 'asm' not in code
    assert code.count('#pragma clang fp contract(off)') == 5          # the four kernels and the helper that states arithmetic
    assert int(re.search(r'kEvdMaxBlocks = (\d+)', text).group(1)) == tempered.MAX_BLOCKS == 64
    assert int(re.search(r'kEvdThreads = (\d+)', text).group(1)) == 256
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, 'ev.hip')
        with open(src, 'w') as f:
            f.write('#include <hip/hip_runtime.h>\n#include <stdint.h>\n#include <math.h>\n#define MSX_MAX_GROUP 64\n#include "{}"\n'.format(
                os.path.join(CSRC, 'evidence_kernels.h')))
        out = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                              '-Rpass-analysis=kernel-resource-usage', '-o', os.path.join(d, 'ev.s'), src],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        asm = open(os.path.join(d, 'ev.s')).read()
    lines = out.stderr.splitlines()
    assert not [ln for ln in lines if 'evidence_kernels.h' in ln and 'warning:' in ln]
    seen = set()
    for i, ln in enumerate(lines):
        m = re.search(r'Function Name: _Z\d+(\w+?_kernel)', ln)
        if m:
            block = '\n'.join(lines[i:i + 14])
            s = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block)
            assert s and int(s.group(1)) == 0, block
            seen.add(m.group(1))
    assert seen == {'evd_part_kernel', 'evd_mean_kernel', 'evd_exp_kernel', 'evd_lme_kernel'}, seen
    assert 'v_fma_f64' not in asm.split('evd_part_kernel')[1].split('.Lfunc_end')[0]      # sums stay sums


def test_the_python_layer_takes_what_the_samplers_pass():
    sig = lambda f: list(inspect.signature(f).parameters)
    assert sig(_lib.Context.tempered_attach_series) == ['self', 'chain', 'dens', 'at_row']
    assert sig(_lib.Series.evidence) == ['self', 'n', 'discard', 'thin', 'col', 'db', 'nblocks']
    p = inspect.signature(tempered.DeviceTemperedSampler.__init__).parameters
    assert p['autocorr'].default == 'host' and p['cap_hint'].default == 0
    from mcmc_spec_amd import mft6
    assert inspect.signature(mft6.device_sampler).parameters['autocorr'].default == 'host'
    for cls in (tempered.TemperedSampler, tempered.DeviceTemperedSampler):
        assert sig(cls.get_autocorr_time)[:2] == ['self', 't'] and inspect.signature(cls.get_autocorr_time).parameters['t'].default == 0
        assert sig(cls.get_summary)[:2] == ['self', 't'] and sig(cls.get_products)[:3] == ['self', 'cols', 't']
        assert sig(cls.mean_log_like) == ['self', 'discard', 'thin']
        assert sig(cls.log_evidence) == ['self', 'discard', 'thin', 'blocks', 'method']
        d = inspect.signature(cls.log_evidence).parameters
        assert (d['discard'].default, d['thin'].default, d['blocks'].default, d['method'].default) == (0, 1, 8, 'ti')
    assert tempered.LogEvidence._fields == ('log_z', 'mc_error', 'ladder_error', 'mean_log_like')
    for word in ('beta_min', 'OMIT', 'Lartillot', 'Xie'):
        assert word in tempered.__doc__, word


def test_bad_options_are_refused_before_anything_touches_a_device():
    with pytest.raises(ValueError):
        tempered.DeviceTemperedSampler(8, 6, None, betas=[1.0, 0.5], autocorr='gpu')
    host = tempered.TemperedSampler(8, 2, lambda q: q[:, 0], lambda q: q[:, 0] * 0, betas=[1.0, 0.5], seed=1)
    with pytest.raises(ValueError):
        host.log_evidence()                    # nothing stored
    with pytest.raises(ValueError):
        host.get_summary()                     # no engine to upload to
    with pytest.raises(ValueError):
        host.get_autocorr_time()               # chain too short
    assert host.get_autocorr_time(t=None, quiet=True).shape == (2, 2)
