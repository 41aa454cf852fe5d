"""CPU: every host-route posterior analysis of the four host sampler families, bit for bit against the recorded results
(tests/golden/analysis_host.npz, made by tests/golden/make_analysis_golden.py): autocorrelation time, split R-hat, moments,
rank R-hat, ESS, MCSE, the parameters of the mode fit and the ladder's evidence -- for the default selection and for
``discard=5, thin=2, cols=[2, 0]``, for all members and for one that is not the first, and what each raises at 3 and at 0
stored rows.  The layer between the samplers and the definitions may change; these numbers and messages may not."""
import importlib.util
import os

import numpy as np
import pytest

import common

GOLDEN = os.path.join(common.ROOT, 'tests', 'golden')


@pytest.fixture(scope='module')
def both():
    spec = importlib.util.spec_from_file_location('make_analysis_golden', os.path.join(GOLDEN, 'make_analysis_golden.py'))
    maker = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(maker)
    with np.load(os.path.join(GOLDEN, 'analysis_host.npz')) as z:
        want = {name: z[name] for name in z.files}
    return maker.record(), want


def test_the_same_analyses_are_recorded_and_computed(both):
    got, want = both
    assert sorted(got) == sorted(want)
    for fam in ('ensemble', 'group', 'tempered', 'group_tempered'):
        for rows in (41, 3, 0):
            assert any(name.startswith('{}:{}:'.format(fam, rows)) for name in want), (fam, rows)
    assert sum(name.endswith('!raise') for name in want) >= 100 and sum(not name.endswith('!raise') for name in want) >= 300


def test_every_number_is_the_recorded_one_bit_for_bit(both):
    got, want = both
    for name in sorted(want):
        if name.endswith('!raise'):
            continue
        g, w = got[name], want[name]
        assert g.dtype == w.dtype and g.shape == w.shape, name
        assert np.array_equal(g, w, equal_nan=w.dtype.kind == 'f'), name


def test_every_raise_is_the_recorded_type_and_message(both):
    got, want = both
    for name in sorted(want):
        if name.endswith('!raise'):
            assert list(got[name]) == list(want[name]), name
