"""CPU: the device chain series and its autocorrelation (include/msx.h, msx_series_*, msx_*sampler_attach_series) are
declared, exported and mirrored; the autocorrelation kernels (csrc/autocorr_kernels.h) compile for gfx950 with no scratch;
the samplers take autocorr=.  No compute calls (no GPU here)."""
import os
import re
import subprocess
import tempfile

import pytest

import common  # noqa: F401
from mcmc_spec_amd import _lib

ROOT = common.ROOT
HDR = os.path.join(ROOT, 'include', 'msx.h')
CSRC = os.path.join(ROOT, 'mcmc_spec_amd', 'csrc')
ENTRIES = {'msx_series_create': 'msx_ctx', 'msx_series_rows': 'msx_series', 'msx_sampler_attach_series': 'msx_ctx',
           'msx_group_sampler_attach_series': 'msx_group', 'msx_series_append': 'msx_series', 'msx_series_read': 'msx_series',
           'msx_series_acf': 'msx_series'}


def test_header_declares_and_library_exports_the_series_entries():
    import __graft_entry__ as ge
    ge.build()
    txt = re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)
    lib = _lib.load()
    for name, first in ENTRIES.items():
        assert re.search(r'\bint ' + name + r'\s*\(\s*' + first + r' \*', txt), name
    assert re.search(r'\bvoid msx_series_destroy\s*\(\s*msx_series \*', txt)
    assert re.search(r'\bconst char \*msx_series_last_error\s*\(\s*msx_series \*', txt)
    for name in list(ENTRIES) + ['msx_series_destroy', 'msx_series_last_error']:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name


def test_autocorrelation_kernels_compile_for_gfx950_without_scratch():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, 'ac.hip')
        with open(src, 'w') as f:
            f.write('#include <hip/hip_runtime.h>\n#include <stdint.h>\n#include "{}"\n'.format(os.path.join(CSRC, 'autocorr_kernels.h')))
        out = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                              '-Rpass-analysis=kernel-resource-usage', '-o', os.path.join(d, 'ac.s'), src],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    seen = set()
    for i, ln in enumerate(lines):
        m = re.search(r'Function Name: _Z\d+(\w+?_kernel)', ln)
        if m:
            block = '\n'.join(lines[i:i + 14])
            s = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block)
            assert s and int(s.group(1)) == 0, block
            seen.add(m.group(1))
    assert seen == {'series_put_kernel', 'series_get_kernel', 'acf_mean_kernel', 'acf_lag_kernel', 'acf_reduce_kernel'}, seen


def test_python_layer_takes_autocorr():
    import inspect
    from mcmc_spec_amd.group import DeviceGroupSampler, GroupSampler, run_group_protocol  # noqa: F401
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    for cls in (DeviceEnsembleSampler, DeviceGroupSampler):
        p = inspect.signature(cls.__init__).parameters['autocorr']
        assert p.default == 'host'
    assert 'k' in inspect.signature(GroupSampler.get_autocorr_time).parameters
    assert DeviceGroupSampler.get_autocorr_time is not GroupSampler.get_autocorr_time
    assert DeviceEnsembleSampler.get_autocorr_time is not DeviceEnsembleSampler.__mro__[1].get_autocorr_time
    assert hasattr(_lib, 'Series') and hasattr(_lib.Context, 'sampler_attach_series') and hasattr(_lib.Group, 'sampler_attach_series')


def test_a_bad_autocorr_mode_is_refused_before_anything_touches_a_device():
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    with pytest.raises(ValueError):
        DeviceEnsembleSampler(8, 2, None, autocorr='gpu')
