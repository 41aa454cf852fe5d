"""The case table of tests/variant_cases.py against the three instance tables of mcmc_spec_amd/csrc/msx.hip: every entry of
kVariants, kPairVariants and kGroupVariants is named by exactly one case, under the name msx_launch_info /
msx_group_launch_info report for it, and no case names anything else -- an instance added without a recipe fails here, on
any machine.  And the probe walkers the GPU matrix tiles its batches with: the oracle must find six of them finite and two
not, or a matrix whose every value is -inf would pass."""
import os
import re

import numpy as np
import pytest

import common
import variant_cases as vc
from common import golden_case

SRC = os.path.join(common.ROOT, 'mcmc_spec_amd', 'csrc', 'msx.hip')
BOOL = '(true|false)'


def _table(text, kind, name):
    i = text.index('const %s %s[] = {' % (kind, name))
    return text[i:text.index('\n};', i)]


def source_names(text=None):
    """(single-context names, group names): what msx_launch_info / msx_group_launch_info build for every table entry."""
    text = open(SRC).read() if text is None else text
    single, groups = [], []
    pat = r'variant<(\d), (\d+), %s, %s, %s, %s(?:, %s)?(?:, (\d))?(?:, %s)?>\("([^"]*)"\)' % ((BOOL,) * 6)
    for ns, threads, gm, sh, pf, lk, r32, full, given, what in re.findall(pat, _table(text, 'Variant', 'kVariants')):
        gm, sh, pf, lk, r32, given = (x == 'true' for x in (gm, sh, pf, lk, r32, given))
        sig = 'NS=%s, %s threads' % (ns, threads)
        sig += ', linked' if lk else ', GM' if gm else ', SH, PF' if pf and sh else ', PF' if pf else ', SH' if sh else ''
        sig += ', R32' if r32 else ''
        sig += {'3': ', FULL', '2': ', FULL(chi2 pass)'}.get(full, '')
        sig += ', GIVEN' if given else ''
        name = 'logprob_kernel<%s> (%s)' % (sig, what)
        single.append(('inpath_recipe_kernel + inpath_conv_kernel + inpath_resample_kernel + ' if given else '') + name)
    for nt, full in re.findall(r'\{logprob_pair_kernel<512, (\d), true(, true)?>, \d, (?:true|false)\}', _table(text, 'PairVariant', 'kPairVariants')):
        single.append(vc.pair('%s element trips per lane%s' % (nt, ', FULL' if full else '')))
    pat = r'group_variant<(\d), (\d+), %s, %s(?:, (\d))?(?:, %s)?>\("([^"]*)"\)' % ((BOOL,) * 3)
    for ns, threads, sh, pf, full, smp, what in re.findall(pat, _table(text, 'GroupVariant', 'kGroupVariants')):
        sh, pf = sh == 'true', pf == 'true'
        sig = 'NS=%s, %s threads' % (ns, threads) + (', SH, PF' if pf and sh else ', PF' if pf else ', SH' if sh else '')
        sig += {'3': ', FULL', '2': ', FULL(chi2 pass)'}.get(full, '')
        groups.append('logprob_group_kernel<%s> (%s)' % (sig, what))
    return single, groups


def compare(cases, names):
    """(entries no case names, names no entry has, entries named more than once)"""
    got = [c.kernel for c in cases]
    return ([n for n in names if n not in got], [g for g in got if g not in names],
            sorted({g for g in got if got.count(g) > 1}))


def test_the_source_tables_parse_whole():
    text = open(SRC).read()
    single, groups = source_names(text)
    assert len(single) == len(set(single)) and len(groups) == len(set(groups))
    # every line of a table that builds an entry was understood
    assert len(single) == _table(text, 'Variant', 'kVariants').count('    variant<') + \
        _table(text, 'PairVariant', 'kPairVariants').count('{logprob_pair_kernel<')
    assert len(groups) == _table(text, 'GroupVariant', 'kGroupVariants').count('    group_variant<')
    assert len(single) == 27 + 4 and len(groups) == 13


@pytest.mark.parametrize('kind', ['single', 'group'])
def test_every_table_entry_has_exactly_one_case(kind):
    names = source_names()[kind == 'group']
    missing, extra, twice = compare([c for c in vc.CASES if c.kind == kind], names)
    assert not missing, 'instances without a case in tests/variant_cases.py: %s' % missing
    assert not extra, 'cases that name no instance of msx.hip: %s' % extra
    assert not twice, 'instances with more than one case: %s' % twice


def test_the_comparison_names_a_missing_and_a_stray_case():
    single, _ = source_names()
    cases = [c for c in vc.CASES if c.kind == 'single']
    gone = vc.by_id('t_gm')
    missing, extra, twice = compare([c for c in cases if c is not gone], single)
    assert missing == [gone.kernel] and not extra and not twice
    stray = gone._replace(kernel=gone.kernel.replace('NS=3', 'NS=4'))
    assert compare(cases + [stray], single) == ([], [stray.kernel], [])
    assert compare(cases + [gone], single) == ([], [], [gone.kernel])


def test_case_ids_and_recipes_are_well_formed():
    ids = [c.id for c in vc.CASES + vc.SAMPLER_CASES]
    assert len(ids) == len(set(ids))
    from mcmc_spec_amd import _lib
    for c in vc.CASES:
        assert c.store in ('f64', 'f32') and c.broadening in ('staging', 'in_path')
        assert c.block in (0, 256, 512, _lib.BLOCK_512_SHARED)
        assert c.path in (_lib.PATH_AUTO, _lib.PATH_FUSED, _lib.PATH_PAIR, _lib.PATH_LINKED, _lib.PATH_INPATH)
        for cus in (64, 256, 304):
            n = c.walkers(cus, 733)
            assert np.sum(n) <= vc.MAX_WALKERS_PER_CU * cus and np.min(n) >= 2 * vc.PROBES
        assert np.max(c.npix) <= 17153          # nothing beyond the smallest spectrum that leaves the LDS
    # the sampler cases plan the group entries the matrix pins, and run an instance of the same stars and threads
    planned = {c.kernel for c in vc.CASES if c.kind == 'group'}
    for s in vc.SAMPLER_CASES:
        assert s.planned in planned and len(s.npix) == 2
        assert s.planned.startswith('logprob_group_kernel<' + s.runs[:len('NS=2, 256 threads')])
        assert ('substituted' in s.id) == (not s.planned.startswith('logprob_group_kernel<%s>' % s.runs))


@pytest.mark.parametrize('which', ['B', 'C'])
def test_the_oracle_finds_six_probes_finite_and_two_not(which):
    c = golden_case(which)
    th = vc.probes(c)
    assert th.shape == (vc.PROBES, 2 * c.nspec + 2) and len({t.tobytes() for t in th}) == vc.PROBES
    post = np.array([common.oracle_logpost(c, t, rad_prior=(c.nspec == 3)) for t in th])
    assert tuple(np.isfinite(post)) == vc.FINITE_AS_POSTERIOR and np.all(np.isneginf(post[6:]))
    # as likelihoods: the box's reject has a value, the walker outside the isochrone raises
    like = np.array([common.oracle_loglike(c, t) for t in th[:7]])
    assert np.all(np.isfinite(like))
    with pytest.raises(ValueError):
        common.oracle_loglike(c, th[7])
    assert len(set(post[:6])) == 6 and len(set(like)) == 7      # eight different walkers, not one value eight times
