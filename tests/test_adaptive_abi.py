"""CPU: the C text of the adaptive ladder against its NumPy definition.  msx_ladder_step is a host
entry that runs the inline functions tempered_adapt_kernel calls, and needs neither a context nor a GPU: the ladder, the
skip flag and the pinned ends must equal ``tempered.ladder_step``'s bit for bit."""
import numpy as np
import pytest

import common  # noqa: F401
import adaptive_numpy as an
from mcmc_spec_amd import _lib, tempered
from mcmc_spec_amd.tempered import default_betas


@pytest.fixture(scope='module', autouse=True)
def built():
    import __graft_entry__ as ge
    ge.build()


def lumpy(T):
    """A hand-made ladder with crowded and empty stretches: gaps that alternate between 1e-3 and 0.5 of what is left."""
    b = [1.0]
    for t in range(1, T):
        b.append(b[-1] * (0.999 if t % 3 else 0.5))
    return np.array(b)


def counts_for(T, nw, kind):
    if kind == 'zero':
        return np.zeros(T - 1, dtype=np.int64)
    if kind == 'all':
        return np.full(T - 1, nw, dtype=np.int64)
    if kind == 'alternating':                       # |dS| at its bound with time = 1, k = 0
        return (np.arange(T - 1) % 2 * nw).astype(np.int64)
    return np.random.default_rng(T).integers(0, nw + 1, T - 1)


@pytest.mark.parametrize('T', [1, 2, 3, 8, 64])
def test_the_host_entry_equals_the_numpy_definition_bit_for_bit(T):
    nw = 50
    ladders = [default_betas(T, 1e-4) if T > 1 else np.array([1.0]), lumpy(T)]
    moved = 0
    for betas in ladders:
        for kind in ('zero', 'all', 'alternating', 'random'):
            counts = counts_for(T, nw, kind)
            for k, lag, time in ((0, 8.0, 1.0), (5, 8.0, 2.0), (77777, 1e4, 100.0)):
                want, wskip = tempered.ladder_step(betas, counts, nw, k, lag, time)
                got, skip = _lib.ladder_step(betas, counts, nw, k, lag, time)
                assert got.tobytes() == want.tobytes(), (T, kind, k)
                assert skip == wskip == 0
                assert got[0] == betas[0] and got[-1] == betas[-1]
                moved += int(not np.array_equal(got, betas))
                if T <= 2:
                    assert np.array_equal(got, betas)
    assert moved == 0 if T <= 2 else moved >= 12     # (equal rates leave a rung where it was only up to a rounding)
    # three times in a row, each step from the last one's ladder: the roundings do not drift apart
    if T > 2:
        a = b = ladders[1]
        for k in range(3):
            counts = counts_for(T, nw, 'random') if k != 1 else counts_for(T, nw, 'alternating')
            a, b = tempered.ladder_step(a, counts, nw, k, 8.0, 1.0)[0], _lib.ladder_step(b, counts, nw, k, 8.0, 1.0)[0]
            assert a.tobytes() == b.tobytes()
        plain, _ = an.ladder_step_plain(ladders[1], counts_for(T, nw, 'random'), nw, 0, 8.0, 1.0)
        assert _lib.ladder_step(ladders[1], counts_for(T, nw, 'random'), nw, 0, 8.0, 1.0)[0].tolist() == plain


def test_a_ladder_built_to_collapse_comes_back_unchanged_with_the_skip_counted():
    b = np.array([1.0, np.nextafter(0.5, 1.0), 0.5, np.nextafter(0.5, 0.0), 0.25])
    counts = np.array([50, 0, 50, 0])
    want, wskip = tempered.ladder_step(b, counts, 50, 0, 8.0, 1.0)
    got, skip = _lib.ladder_step(b, counts, 50, 0, 8.0, 1.0)
    assert skip == wskip == 1 and got.tobytes() == want.tobytes() == b.tobytes()


@pytest.mark.parametrize('lag,time', [(0.0, 2.0), (-1.0, 2.0), (float('nan'), 2.0), (float('inf'), 2.0), (8.0, 0.5), (8.0, float('nan')),
                                      (8.0, float('inf'))])
def test_the_host_entry_refuses_what_the_definition_refuses(lag, time):
    with pytest.raises(ValueError):
        _lib.ladder_step([1.0, 0.5, 0.25], [1, 2], 12, 0, lag, time)
    with pytest.raises(ValueError):
        tempered.ladder_step([1.0, 0.5, 0.25], [1, 2], 12, 0, lag, time)
