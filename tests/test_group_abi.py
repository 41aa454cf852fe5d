"""CPU: the target-group entry points (include/msx.h, msx_group_*) are declared, exported and mirrored, and every instance
of the group kernel keeps its working set in registers.  No compute calls (no GPU here)."""
import os
import re
import subprocess
import tempfile

import common  # noqa: F401
from mcmc_spec_amd import _lib

ROOT = common.ROOT
HDR = os.path.join(ROOT, 'include', 'msx.h')
GROUP_ENTRIES = ['msx_group_create', 'msx_group_destroy', 'msx_group_last_error', 'msx_group_logprob_batch',
                 'msx_group_logprob_batch_dev', 'msx_group_launch_info']


def test_header_declares_and_library_exports_the_group_entries():
    import __graft_entry__ as ge
    ge.build()
    txt = re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)
    assert 'typedef struct msx_group msx_group;' in txt
    lib = _lib.load()
    for name in GROUP_ENTRIES:
        assert re.search(r'\b' + name + r'\s*\(', txt), name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name


def test_max_group_is_mirrored():
    m = re.search(r'#define MSX_MAX_GROUP (\d+)', open(HDR).read())
    assert m and int(m.group(1)) == _lib.MAX_GROUP == 64


def test_group_kernel_instances_use_no_scratch():
    """Every instance of logprob_group_kernel: scratch 0 (the member's problem is read through the constant address space,
    the member index stays in scalar registers), and the table of instances covers binaries and triples, 256 / 512 threads."""
    src = os.path.join(ROOT, 'mcmc_spec_amd', 'csrc', 'msx.hip')
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, 't.s')
        out = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                              '-mllvm', '-amdgpu-kernarg-preload-count=8',
                              '-Rpass-analysis=kernel-resource-usage', '-o', asm, src],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
    lines = out.stderr.splitlines()
    seen = set()
    for i, ln in enumerate(lines):
        if 'Function Name' in ln and 'logprob_group_kernel' in ln:
            block = '\n'.join(lines[i:i + 14])
            m = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block)
            assert m and int(m.group(1)) == 0, block
            seen.add(re.search(r'logprob_group_kernelILi(\d)ELi(\d+)E', ln).groups())
    assert seen == {('2', '256'), ('2', '512'), ('3', '256'), ('3', '512')}, seen
