"""CPU: the target group's device-resident sampler (include/msx.h, msx_group_sampler_*) is declared, exported and mirrored,
and every instance of the group kernel -- the plain ones and the sampler's (SMP) -- keeps its working set in registers.
No compute calls (no GPU here)."""
import os
import re
import subprocess
import tempfile

import common  # noqa: F401
from mcmc_spec_amd import _lib

ROOT = common.ROOT
HDR = os.path.join(ROOT, 'include', 'msx.h')
CHAIN_ENTRIES = ['msx_group_sampler_begin', 'msx_group_sampler_enqueue', 'msx_group_sampler_collect', 'msx_group_sampler_end']


def test_header_declares_and_library_exports_the_group_sampler_entries():
    import __graft_entry__ as ge
    ge.build()
    txt = re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)
    lib = _lib.load()
    for name in CHAIN_ENTRIES:
        assert re.search(r'\bint ' + name + r'\s*\(\s*msx_group \*', txt), name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name


def test_python_layer_has_the_device_group_sampler():
    from mcmc_spec_amd.group import DeviceGroupSampler, GroupSampler
    for name in ('sample', 'run_mcmc', 'reset', 'get_chain', 'get_log_prob', 'acceptance_fraction'):
        assert hasattr(DeviceGroupSampler, name), name
    assert issubclass(DeviceGroupSampler, GroupSampler)


def test_group_kernel_instances_with_the_sampler_use_no_scratch():
    """Every instance of logprob_group_kernel, the sampler's (last template argument true) among them: scratch 0."""
    src = os.path.join(ROOT, 'mcmc_spec_amd', 'csrc', 'msx.hip')
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, 't.s')
        out = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                              '-mllvm', '-amdgpu-kernarg-preload-count=8',
                              '-Rpass-analysis=kernel-resource-usage', '-o', asm, src],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    plain, smp = set(), set()
    for i, ln in enumerate(lines):
        if 'Function Name' in ln and 'logprob_group_kernel' in ln:
            block = '\n'.join(lines[i:i + 14])
            m = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block)
            assert m and int(m.group(1)) == 0, block
            args, is_smp = re.search(r'logprob_group_kernelI(\w+?)ELb([01])EEEv', ln).groups()
            (smp if is_smp == '1' else plain).add(args)
    assert len(plain) == 13, sorted(plain)
    # (three entries have no sampler instance -- as one they spilled -- and the sampler takes a neighbour there)
    assert smp <= plain and len(smp) == 10, sorted(smp)
