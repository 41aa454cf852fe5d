"""CPU: the high-precision twin of the Gaussian broadening (tests/broaden_numpy.py) against NumPy's convolution and the
oracle's restatement of pyasl.instrBroadGaussFast, and the evidence that its checker would notice a subtly wrong kernel:
float64 emulations of the kernels' summation order pass ``check`` on every case of tests/test_gpu_broaden_shapes.py, and
four deliberately wrong emulations each fail it on the cases named here.  No wrong kernel ever runs on a GPU for this."""
import numpy as np
import pytest

import common  # noqa: F401
import broaden_numpy as bn
from oracle import mft6_oracle as orc

LONGEST = ('longest', bn.N_LONGEST, None, 5.0, lambda lx, n: 8900 <= lx <= bn.MAX_LX)
IDS = [c[0] for c in bn.CASES]


def _case(cid):
    if cid == 'longest':
        return LONGEST[:2] + (bn.longest_resolution(),) + LONGEST[3:]
    return next(c for c in bn.CASES if c[0] == cid)


def test_long_double_is_wider_than_double():
    assert np.finfo(bn.LD).eps < 2.0 ** -60


def _fits(cid):
    case = _case(cid)
    n, dx, sigma, lx = bn.case_params(case)
    return case, n, dx, sigma, lx


FITS = [c for c in IDS if _fits(c)[4] <= _fits(c)[1]]     # lx <= n: where np.convolve(..., 'same') has n samples


def _ulps_of_mag(got, ref, mag):
    """max |got - ref| / (2^-52 mag), in long double (0 where mag vanishes)."""
    u = bn.LD(2.0 ** -52) * mag
    return float(np.max(np.where(u > 0, np.abs(np.asarray(got).astype(bn.LD) - ref) / np.where(u > 0, u, 1), np.abs(got))))


@pytest.mark.parametrize('cid', IDS)
def test_lx_of_is_the_oracles_kernel_length(cid):
    case, n, dx, sigma, lx = _fits(cid)
    wl = bn.axis(n)
    assert lx == len(orc.broad_gauss_kernel(wl[1] - wl[0], bn.sigma_of(np.mean(wl), case[2]), case[3]))


@pytest.mark.parametrize('cid', FITS)
def test_twin_equals_numpy_convolve(cid):
    """np.convolve(y, float64 taps of the twin, 'same'): 4 ulp of mag (measured: at most 3.995, lx = 1292)."""
    case, n, dx, sigma, lx = _fits(cid)
    e = bn.taps(dx, sigma, lx)
    for row in bn.rows(n)[1:]:
        ref, mag = bn.conv_same(row, e)
        assert _ulps_of_mag(np.convolve(row, e.astype(float), 'same'), ref, mag) <= 4.0


@pytest.mark.parametrize('cid', FITS)
def test_twin_equals_the_oracle_to_4_ulp(cid):
    """The definition -- centre, zero padding, length -- against the oracle's instr_broad_gauss_fast, odd and even lx: within
    4 ulp of mag when both convolve the SAME taps, the oracle's float64 ones (measured: at most 3.45).

    The taps are compared on their own (test_taps_follow_broad_gauss_fast_for_odd_and_even_lengths): the oracle's are
    float64 ``1 / sqrt(2 pi sigma^2) exp(-x^2 / 2 sigma^2)`` over their float64 sum, 6 to 13 ulp from the long-double ones
    in the wings, where rounding x^2 / 2 sigma^2 ~ 12 is amplified by the exponential.  With the long-double taps on the
    twin's side the oracle is 4.16 ulp away on 'n1027' (lx = 31; 4.2 to 4.75 on this table for other seeds of the rows), so
    4 ulp is a statement about one set of taps; end to end the oracle is held to the bound that ``check`` derives for a
    float64 implementation (test_twin_equals_the_oracle_within_the_derived_bound)."""
    case, n, dx, sigma, lx = _fits(cid)
    wl = bn.axis(n)
    e = orc.broad_gauss_kernel(wl[1] - wl[0], bn.sigma_of(np.mean(wl), case[2]), case[3])
    assert len(e) == lx
    for row in bn.rows(n)[1:]:
        ref, mag = bn.conv_same(row, e)
        got = orc.instr_broad_gauss_fast(wl, row, case[2], maxsig=case[3])
        assert got.shape == (n,)
        ulps = _ulps_of_mag(got, ref, mag)
        print(cid, 'lx', lx, 'oracle against the twin on the same taps:', ulps, 'ulp of mag')
        assert ulps <= 4.0, (cid, lx, ulps)


@pytest.mark.parametrize('cid', FITS)
def test_twin_equals_the_oracle_within_the_derived_bound(cid):
    """... and inside the bound ``check`` sets for a float64 implementation: the same definition, odd and even lx (a
    sample one position off is 1e-2 away, thirteen orders above it)."""
    case, n, dx, sigma, lx = _fits(cid)
    wl = bn.axis(n)
    for row in bn.rows(n)[1:]:
        assert bn.check(orc.instr_broad_gauss_fast(wl, row, case[2], maxsig=case[3]), row, dx, sigma, lx, patched=False) <= 0.5
        assert bn.check(orc.broaden(wl, row, case[2])[1] if case[3] == 5.0 else bn.patch(orc.instr_broad_gauss_fast(
            wl, row, case[2], maxsig=case[3])), row, dx, sigma, lx, patched=True) <= 0.5


def test_taps_follow_broad_gauss_fast_for_odd_and_even_lengths():
    for lx in (1, 2, 31, 60, 89, 90):
        want = orc.broad_gauss_kernel(0.2, 1.7, maxsig=(lx - 1 + 0.5) * 0.2 / (2 * 1.7))
        assert len(want) == lx
        assert np.max(np.abs(bn.taps(0.2, 1.7, lx).astype(float) - want)) <= 4 * 2.0 ** -52 * want.max()
    # an even kernel is off centre: its peak is tap lx / 2 - 1, and c = (lx - 1) // 2 puts that tap on the sample itself
    e = bn.taps(0.2, 1.7, 60)
    assert int(np.argmax(e)) == 29 == bn.off0_of(60) == bn.centre_of(60)


@pytest.mark.parametrize('cid', ['n16', 'n64', 'n300', 'lds_attribute'])
def test_numpy_same_returns_the_longer_length(cid):
    """A kernel longer than the row: np.convolve(y, e, 'same') returns max(n, lx) samples, so the reference's ``broaden``
    returns a flux longer than its wavelengths.  The library returns the n samples of the definition."""
    case = _case(cid)
    n, dx, sigma, lx = bn.case_params(case)
    wl, y, _ = bn.rows(n)
    assert lx > n
    got = orc.instr_broad_gauss_fast(wl, y, case[2], maxsig=case[3])
    assert got.shape == (lx,)
    ww, b = orc.broaden(wl, y, case[2]) if case[3] == 5.0 else (wl, got)
    assert len(b) == lx != len(ww) == n
    # ... and the definition's n samples are the middle of NumPy's full convolution, not a slice 'same' would name
    full = np.convolve(y, bn.taps(dx, sigma, lx).astype(float), 'full')
    c = bn.centre_of(lx)
    ref, mag = bn.conv_same(y, bn.taps(dx, sigma, lx))
    assert np.all(np.abs(full[c:c + n] - ref.astype(float)) <= (lx + 4) * bn.U * mag.astype(float))


@pytest.mark.parametrize('cid', IDS + ['longest'])
def test_emulations_of_the_kernels_stay_inside_the_bound(cid):
    n, dx, sigma, lx = bn.case_params(_case(cid))
    _, y, yz = bn.rows(n)
    worst = 0.0
    for row in (y, yz):
        out = bn.emulate(row, dx, sigma, lx)
        worst = max(worst, bn.check(bn.patch(out), row, dx, sigma, lx, patched=True), bn.check(out, row, dx, sigma, lx, patched=False))
    print(cid, 'lx', lx, 'float64 emulation: worst error / bound', worst)
    assert worst <= 0.5
    if lx == 1:
        assert np.array_equal(bn.emulate(y, dx, sigma, lx), y)


def test_emulation_of_the_inpath_composite_stays_inside_the_bound():
    """The in-path kernel convolves sum_star sum_corner w row: the composite is its input, the bound the same."""
    rng = np.random.default_rng(12)
    for cid in ('n1025_two_trips', 'n1027', 'n2049_even', 'n300'):
        n, dx, sigma, lx = bn.case_params(_case(cid))
        rows8 = np.stack([bn.rows(n)[1] * (1.0 + 0.1 * k) + 0.02 * rng.normal(size=n) for k in range(8)])
        w8 = rng.uniform(0.0, 1.0, size=8) * 1e-19
        comp = bn.composite(rows8, w8)
        assert bn.check(bn.emulate(comp, dx, sigma, lx), comp, dx, sigma, lx, patched=False) <= 0.5


# which cases catch which mistake ('tail' is the in-path kernel's: its guarded stores o + j < n)
ODD = {'identity', 'n1023', 'n1027'}
MUTANTS = {
    'centre': set(IDS),                                            # every case, the identity included
    'off0': {c for c in IDS if c not in ODD},                      # even lx only: the odd formula is right for odd lx
    'halo': {c for c in IDS if c not in ODD},                      # lx - 1 - c == c for odd lx
    'tail': {c[0] for c in bn.CASES if c[1] % 4 != 0},             # every n that is no multiple of 4
}


@pytest.mark.parametrize('mutant', sorted(MUTANTS))
def test_a_subtly_wrong_kernel_fails_the_check(mutant):
    caught = set()
    for case in bn.CASES:
        n, dx, sigma, lx = bn.case_params(case)
        _, y, _ = bn.rows(n)
        out = bn.emulate(y, dx, sigma, lx, mutant=mutant)
        try:
            bn.check(out, y, dx, sigma, lx, patched=False)
        except AssertionError:
            caught.add(case[0])
    print(mutant, 'caught by', sorted(caught))
    assert caught == MUTANTS[mutant] and caught
    # the cases on each side of a tile seam are among them
    assert caught & {'n1023', 'n1024_even', 'n1025_two_trips', 'n1027', 'n2049_even'}


def test_the_odd_cases_are_odd():
    for case in bn.CASES:
        lx = bn.case_params(case)[3]
        assert (lx % 2 == 1) == (case[0] in ODD), (case[0], lx)


def test_the_patch_is_noticed():
    n, dx, sigma, lx = bn.case_params(_case('n1027'))
    _, y, _ = bn.rows(n)
    out = bn.patch(bn.emulate(y, dx, sigma, lx))
    assert bn.check(out, y, dx, sigma, lx, patched=True) <= 0.5
    for i, src in ((4, 6), (n - 10, n - 12), (n - 1, n - 1)):   # a patch one sample short, or taken from the neighbour
        bad = out.copy()
        bad[i] = bn.emulate(y, dx, sigma, lx)[src]
        with pytest.raises(AssertionError):
            bn.check(bad, y, dx, sigma, lx, patched=True)


def test_limits_of_the_launch_code():
    assert bn.lds_bytes(bn.MAX_LX) <= 150 * 1024 < bn.lds_bytes(bn.MAX_LX + 1)
    assert 8900 <= bn.params(bn.N_LONGEST, bn.longest_resolution(), 5.0)[2] <= bn.MAX_LX
    assert bn.params(bn.N_LONGEST, bn.refused_resolution(), 5.0)[2] > bn.MAX_LX


def test_resample_restatement_is_interp1d_bit_for_bit():
    """resample_kernel's arithmetic in NumPy against scipy's interp1d on the GPU test's inputs: duplicated knots, queries on
    every knot and at both ends -- equality is the condition the device is held to, not a tolerance."""
    from scipy.interpolate import interp1d
    xs, ys, xq = bn.resample_inputs()
    assert len(xq) == 1392 and np.array_equal(bn.resample_numpy(xs, ys, xq), interp1d(xs, ys)(xq))
    x2, y2 = np.array([1.0, 2.5]), np.array([0.3, -1.7])
    q2 = np.concatenate([[1.0, 2.5], np.random.default_rng(1).uniform(1.0, 2.5, size=50)])
    assert np.array_equal(bn.resample_numpy(x2, y2, q2), interp1d(x2, y2)(q2))
