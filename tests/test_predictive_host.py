"""CPU: the NumPy twin of the posterior predictive check (tests/predictive_numpy.py) against values worked out by hand on a
3-sample x 2-row x 5-pixel array -- the twin is what the GPU tests compare the device with, so it is pinned here first."""
import numpy as np

import common  # noqa: F401  (puts the repository on sys.path)
import predictive_numpy as twin

# sample, row, pixel
S = np.array([[[1.0, 2.0, 3.0, 4.0, 5.0], [10.0, 10.0, 10.0, 10.0, 10.0]],
              [[3.0, 2.0, 1.0, 0.0, -1.0], [20.0, 40.0, 10.0, 10.0, 16.0]],
              [[2.0, 5.0, 5.0, 8.0, 2.0], [60.0, 10.0, 10.0, 40.0, 13.0]]])


def test_band_by_hand():
    out = twin.reduce(S, q=(0.0, 0.25, 0.5, 1.0))
    assert out['count'] == 3
    assert np.array_equal(out['mean'], [[2.0, 3.0, 3.0, 4.0, 2.0], [30.0, 20.0, 10.0, 20.0, 13.0]])
    # sum (x - mean)^2 / 2
    assert np.array_equal(out['var'], [[1.0, 3.0, 4.0, 16.0, 9.0], [700.0, 300.0, 0.0, 300.0, 9.0]])
    assert np.array_equal(out['min'], [[1.0, 2.0, 1.0, 0.0, -1.0], [10.0, 10.0, 10.0, 10.0, 10.0]])
    assert np.array_equal(out['max'], [[3.0, 5.0, 5.0, 8.0, 5.0], [60.0, 40.0, 10.0, 40.0, 16.0]])
    assert np.array_equal(out['quantiles'][0], out['min']) and np.array_equal(out['quantiles'][3], out['max'])
    # q = 0.5 with three samples: h = 1 falls exactly on the middle element
    assert np.array_equal(out['quantiles'][2], [[2.0, 2.0, 3.0, 4.0, 2.0], [20.0, 10.0, 10.0, 10.0, 13.0]])
    # q = 0.25: h = 0.5, half way between the two smallest
    assert np.array_equal(out['quantiles'][1], [[1.5, 2.0, 2.0, 2.0, 0.5], [15.0, 10.0, 10.0, 10.0, 11.5]])
    assert np.array_equal(twin.two_pass_var(S), out['var'])


def test_a_sample_that_could_not_be_evaluated_is_left_out():
    bad = S.copy()
    bad[1] = np.nan
    out = twin.reduce(bad, q=(0.5,), status=[0, 4, 0])
    assert out['count'] == 2
    assert np.array_equal(out['mean'], [[1.5, 3.5, 4.0, 6.0, 3.5], [35.0, 10.0, 10.0, 25.0, 11.5]])
    assert np.array_equal(out['var'], [[0.5, 4.5, 2.0, 8.0, 4.5], [1250.0, 0.0, 0.0, 450.0, 4.5]])
    assert np.array_equal(out['quantiles'][0], out['mean'])   # two samples: the median is their mean
    assert np.array_equal(out['min'][0], [1.0, 2.0, 3.0, 4.0, 2.0]) and np.array_equal(out['max'][1], [60.0, 10.0, 10.0, 40.0, 13.0])


def test_count_one_and_zero():
    one = twin.reduce(S, q=(0.16, 0.84), status=[1, 0, 2])
    assert one['count'] == 1 and np.all(np.isnan(one['var']))
    for name in ('mean', 'min', 'max'):
        assert np.array_equal(one[name], S[1])
    assert np.array_equal(one['quantiles'], np.stack([S[1], S[1]]))
    none = twin.reduce(S, q=(0.16, 0.84), status=[1, 4, 2])
    assert none['count'] == 0 and none['quantiles'].shape == (2, 2, 5)
    for name in ('mean', 'var', 'min', 'max', 'quantiles'):
        assert np.all(np.isnan(none[name])), name


def test_two_pass_variance_survives_a_large_offset():
    """1e8 + {0, 1, 2}: the variance is exactly 1; sums of raw squares (about 1e16, spacing 2) cannot hold it."""
    x = (1e8 + np.array([0.0, 1.0, 2.0]))[:, None, None]
    assert twin.two_pass_var(x)[0, 0] == 1.0
    naive = (np.sum(x ** 2) - np.sum(x) ** 2 / 3) / 2
    assert naive != 1.0
