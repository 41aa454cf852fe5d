"""The launch plan pinned: which variant, block, dynamic LDS, grid, sub-batch and requested bytes the library's
``msx_launch_info`` / ``msx_bytes_per_eval`` report, over the matrix of ``tests/golden/make_launch_plans.py``, against
``tests/golden/launch_plans.json`` (generated with the library before the launch decision was gathered into one plan);
and what ``msx_group_launch_info`` reports for the group matrix, against ``tests/golden/group_launch_plans.json``
(generated with the library before the group planner was made to share the fused form's rules)."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

import make_launch_plans as mlp  # noqa: E402

SRC = os.path.join(ROOT, 'mcmc_spec_amd', 'csrc', 'msx.hip')


def _table(name):
    text = open(SRC).read()
    i = text.index('const %s %s[] = {' % (name[0], name[1]))
    return text[i:text.index('\n};', i)]


def test_fixture_covers_every_variant():
    """Every logprob_kernel entry of kVariants, and every pair-kernel entry, is some case's kernel."""
    kernels = {c['launch_info']['kernel'] for c in mlp.load() if 'kernel' in c.get('launch_info', {})}
    entries = re.findall(r'variant<(\d), (\d+),[^>]*>\("([^"]*)"\)', _table(('Variant', 'kVariants')))
    assert len(entries) == 27 and len(set(entries)) == len(entries)
    for ns, threads, what in entries:
        assert any(f'logprob_kernel<NS={ns}, {threads} threads' in k and k.endswith(f'({what})') for k in kernels), what
    pairs = re.findall(r'logprob_pair_kernel<512, (\d), true(, true)?>', _table(('PairVariant', 'kPairVariants')))
    assert len(pairs) == 4
    for nt, full in pairs:
        assert any(k.startswith(f'pair_plan_kernel + logprob_pair_kernel<512 threads, {nt} element trips per lane'
                                + (', FULL>' if full else '>')) for k in kernels), (nt, full)


def test_group_fixture_covers_every_group_variant():
    """Every entry of kGroupVariants is some group case's kernel."""
    kernels = {c['launch_info']['kernel'] for c in mlp.load_groups() if 'kernel' in c['launch_info']}
    entries = re.findall(r'group_variant<(\d), (\d+), (true|false), (true|false)(?:, (\d))?[^>]*>\("([^"]*)"\)',
                         _table(('GroupVariant', 'kGroupVariants')))
    assert len(entries) == 13 and len(set(entries)) == len(entries)
    for ns, threads, sh, pf, full, what in entries:
        flags = {('true', 'true'): ', SH, PF', ('false', 'true'): ', PF', ('true', 'false'): ', SH'}.get((sh, pf), '')
        flags += {'3': ', FULL', '2': ', FULL(chi2 pass)'}.get(full, '')
        assert f'logprob_group_kernel<NS={ns}, {threads} threads{flags}> ({what})' in kernels, (ns, threads, sh, pf, full)


@pytest.mark.gpu
def test_group_launch_plans_match_the_fixture():
    want = mlp.load_groups()
    got = mlp.collect_groups()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g == w


@pytest.mark.gpu
def test_launch_plans_match_the_fixture():
    want = mlp.load()
    got = mlp.collect()
    assert len(got) == len(want)
    for g, w in zip(got, want):
        if g.get('path') == 'inpath':
            # msx_bytes_per_eval used to price the fused variant for the in-path form; it now reads the same plan as
            # msx_launch_info
            assert g['bytes_per_eval'] == g['launch_info']['requested_bytes_per_eval']
            g, w = dict(g, bytes_per_eval=None), dict(w, bytes_per_eval=None)
        assert g == w
