"""CPU: the C ABI of the posterior predictive check (include/msx.h: msx_predictive_batch, msx_series_predictive) -- the
exports and their argument counts, the new kernels' freedom from scratch memory, and the refusals that need no device."""
import ctypes
import os
import re
import subprocess
import tempfile

import common
from mcmc_spec_amd import _lib

ROOT = common.ROOT
NEW = {'msx_predictive_batch': 13, 'msx_series_predictive': 14}


def test_new_entry_points_are_declared_exported_and_bound():
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load()
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'msx.h')).read(), flags=re.S)
    for name, nargs in NEW.items():
        m = re.search(r'\bint ' + name + r'\s*\((.*?)\)\s*;', hdr, flags=re.S)
        assert m, name
        assert len(m.group(1).split(',')) == nargs, name
        assert name in _lib.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == nargs, name


def test_the_python_layer_names_the_terms_in_the_headers_order():
    from mcmc_spec_amd import predictive
    assert predictive.TERM_NAMES == ('chi_spec', 'chi_contrast', 'chi_phot', 'chi_total')
    hdr = open(os.path.join(ROOT, 'include', 'msx.h')).read()
    assert 'terms [n][4]: chi_spec, chi_contrast, chi_phot, chi_total' in hdr


def test_null_handles_are_refused_without_a_device():
    lib = _lib.load()
    d = (ctypes.c_double * 8)()
    i32 = (ctypes.c_int32 * 2)()
    i64 = (ctypes.c_int64 * 2)()
    assert lib.msx_predictive_batch(None, d, 1, 6, d, 1, 0, d, d, d, d, i32, i64) == _lib.MSX_ERR_INVALID
    assert lib.msx_series_predictive(None, None, 1, 0, 1, d, 1, 0, d, d, d, None, i64, i32) == _lib.MSX_ERR_INVALID


def test_predictive_kernels_use_no_scratch_memory():
    """The sample and fill kernels (binary, triple) and the reduce kernel keep a sample's recipe and their partial sums in
    LDS and registers: ScratchSize 0 and not one scratch instruction (read as tests/test_products_abi.py reads it)."""
    src = os.path.join(ROOT, 'mcmc_spec_amd', 'csrc', 'msx.hip')
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, 't.s')
        out = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                              '-mllvm', '-amdgpu-kernarg-preload-count=8', '-Rpass-analysis=kernel-resource-usage', '-o', asm, src],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        text = open(asm).read()
    lines = out.stderr.splitlines()
    seen = []
    for i, ln in enumerate(lines):
        if 'Function Name' in ln and re.search(r'predictive_(sample|fill|reduce)_kernel', ln):
            block = '\n'.join(lines[i:i + 14])
            m = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block)
            assert m and int(m.group(1)) == 0, block
            name = re.search(r'Function Name: (\S+)', ln).group(1)
            body = text[text.index('\n' + name + ':'):]
            body = body[:body.index('.Lfunc_end')]
            assert 'scratch_' not in body, name
            seen.append(name)
    assert len(seen) == 5, seen   # sample and fill, binary and triple; reduce
