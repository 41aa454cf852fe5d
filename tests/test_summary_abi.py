"""CPU: the posterior summaries of a device chain series (include/msx.h, msx_series_order_stats / _hist / _hist2d;
DESIGN.md section 14) are declared, exported and mirrored; their kernels (csrc/summary_kernels.h) compile for gfx950 with
no scratch; the host interpolation of summary.quantiles is np.quantile's; bad arguments are refused before a device is
touched.  No compute calls (no GPU here)."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import common  # noqa: F401
from mcmc_spec_amd import _lib
from summary_numpy import loop_counts, numpy_counts, reference_counts

ROOT = common.ROOT
HDR = os.path.join(ROOT, 'include', 'msx.h')
CSRC = os.path.join(ROOT, 'mcmc_spec_amd', 'csrc')
ENTRIES = ['msx_series_order_stats', 'msx_series_hist', 'msx_series_hist2d']


def test_header_declares_and_library_exports_the_summary_entries():
    import __graft_entry__ as ge
    ge.build()
    txt = re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r'\bint ' + name + r'\s*\(\s*msx_series \*', txt), name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name
    m = re.search(r'#define MSX_COL_RATIO\(a, b\) \((0x[0-9a-f]+)u \| \(\(uint32_t\)\(a\) << (\d+)\) \| \(uint32_t\)\(b\)\)', txt)
    assert m, 'MSX_COL_RATIO'
    assert _lib.col_ratio(4, 3) == int(m.group(1), 16) | (4 << int(m.group(2))) | 3


def test_summary_kernels_compile_for_gfx950_without_scratch():
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, 'sk.hip')
        with open(src, 'w') as f:
            f.write('#include <hip/hip_runtime.h>\n#include <stdint.h>\n#include "{}"\n#include "{}"\n#include "{}"\n'.format(
                HDR, os.path.join(CSRC, 'wave_ops.h'), os.path.join(CSRC, 'summary_kernels.h')))
        out = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                              '-Rpass-analysis=kernel-resource-usage', '-o', os.path.join(d, 'sk.s'), src],
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
    assert seen == {'sel_pass_kernel', 'sel_pick_kernel', 'hist_kernel', 'hist2d_kernel'}, seen


def test_python_layer_has_the_summary_methods():
    import inspect
    from mcmc_spec_amd import summary
    from mcmc_spec_amd.group import DeviceGroupSampler
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    for name in ('order_stats', 'hist', 'hist2d'):
        assert callable(getattr(_lib.Series, name)), name
    p = inspect.signature(DeviceEnsembleSampler.get_summary).parameters
    assert p['q'].default == (0.16, 0.5, 0.84) and p['discard'].default == 0 and p['thin'].default == 1 and p['cols'].default is None
    p = inspect.signature(DeviceGroupSampler.get_summary).parameters
    assert p['k'].default is None and p['q'].default == (0.16, 0.5, 0.84)
    for name in ('quantiles', 'medians', 'marginals', 'corner_counts', 'summarize', 'col_ratio'):
        assert callable(getattr(summary, name)), name
    assert inspect.signature(summary.marginals).parameters['nbins'].default == 75
    assert inspect.signature(summary.corner_counts).parameters['bins'].default == 50


class SortedStub:
    """What summary.quantiles needs of a series, answered from NumPy: members of counts[m] walkers over one column each."""

    def __init__(self, samples):
        self.samples = [np.sort(np.asarray(s, dtype=float)) for s in samples]   # member m's flat sample of the only column
        self.k, self.ndim = len(samples), 1
        self.counts = np.array([len(s) for s in samples], dtype=np.int64)        # (one row: N_m = the member's walkers)
        self.calls = 0

    def order_stats(self, n, discard, thin, cols, ranks):
        assert (n, discard, thin, list(cols)) == (1, 0, 1, [0])
        self.calls += 1
        ranks = np.asarray(ranks)
        assert ranks.shape[0] == self.k and all(np.all((ranks[m] >= 0) & (ranks[m] < self.counts[m])) for m in range(self.k))
        return np.stack([self.samples[m][ranks[m]] for m in range(self.k)])[:, None, :], self.counts


def test_quantile_interpolation_is_numpys_bit_for_bit():
    from mcmc_spec_amd import summary
    rng = np.random.default_rng(11)
    q = [0.0, 0.025, 0.16, 0.5, 0.84, 0.975, 1.0]
    sizes = [2, 3, 4, 5, 7, 50, 51, 750, 4999, 5000] + list(rng.integers(2, 5001, size=90))
    samples = [rng.normal(size=int(s)) * 10.0 ** rng.integers(-5, 6) + rng.normal() * 3.0 for s in sizes]
    samples.append(np.repeat(rng.normal(size=40), rng.integers(1, 30, size=40)))     # runs of equal values, as a chain has
    samples.append(np.full(17, 2.5))
    for lo in range(0, len(samples), 8):    # several members of different sizes per call: ranks differ per member
        part = samples[lo:lo + 8]
        stub = SortedStub(part)
        got = summary.quantiles(stub, 1, q)
        assert stub.calls == 1 and got.shape == (len(part), 1, len(q))
        for m, s in enumerate(part):
            assert np.array_equal(got[m, 0], np.quantile(s, q)), (lo, m)
            assert np.array_equal(got[m, 0, [2, 3, 4]], np.percentile(s, [16, 50, 84])), (lo, m)


def test_medians_are_numpys_bit_for_bit():
    from mcmc_spec_amd import summary
    rng = np.random.default_rng(12)
    samples = [rng.normal(size=int(s)) * 1e3 + 7.0 for s in [1, 2, 3, 4, 750, 751, 3894]] + [np.full(6, -1.5)]
    stub = SortedStub(samples)
    got = summary.medians(stub, 1)
    both = summary.summary_of(stub, 1)
    for m, s in enumerate(samples):
        assert got[m, 0] == np.median(s) and both['median'][m, 0] == np.median(s), m
        assert both['min'][m, 0] == s.min() and both['max'][m, 0] == s.max() and both['count'][m] == s.size
        assert np.array_equal(both['quantiles'][m, 0], np.quantile(s, [0.16, 0.5, 0.84])), m
    assert stub.calls == 2


def test_bad_arguments_are_refused_before_anything_touches_a_device():
    from mcmc_spec_amd import summary

    class Untouchable:
        k, ndim, counts = 1, 2, np.array([4])

        def __getattr__(self, name):
            raise AssertionError('the series was touched: ' + name)

    s = Untouchable()
    for q in ([-0.01], [0.5, 1.5], [np.nan], []):
        with pytest.raises(ValueError):
            summary.quantiles(s, 10, q)
        with pytest.raises(ValueError):
            summary.summarize(np.zeros((3, 4, 2)), None, q=q)
    with pytest.raises(ValueError):
        summary.marginals(s, 10, [0], nbins=1)
    with pytest.raises(ValueError):
        summary.marginals(s, 10, [0], rule='corner')
    with pytest.raises(ValueError):
        summary.corner_counts(s, 10, [0, 1], bins=129)
    with pytest.raises(ValueError):
        summary.quantiles(s, 5, [0.5], discard=5)        # an empty selection
    with pytest.raises(ValueError):
        summary.summarize(np.zeros((3, 4, 2)), None, marginal={'cols': [0], 'rule': 'corner'})
    with pytest.raises(ValueError):
        _lib.col_ratio(256, 0)


def test_the_restatements_are_the_references_loop():
    """searchsorted(edges, x, 'right') - 1 with the indices >= nbins - 1 dropped IS the double loop of mft6.py:2046-2049, on
    values next to np.linspace edges too; np.histogram differs from it only in the values ON the last edge."""
    rng = np.random.default_rng(3)
    x = rng.normal(size=3000)
    edges = np.linspace(x.min(), x.max(), 75)
    x = np.concatenate([x, edges, np.nextafter(edges, -np.inf), np.nextafter(edges, np.inf)])
    want = loop_counts(x, edges)
    assert want[-1] == 0 and np.array_equal(reference_counts(x, edges), want)
    on_last = int(np.sum(x == edges[-1]))
    assert on_last >= 2
    h = numpy_counts(x, edges)
    assert np.array_equal(h[:-1], want[:-2]) and h[-1] == want[-2] + on_last
