"""CPU: the NumPy restatement of the rotational broadening (tests/rotbroad_numpy.py) against properties that do not
depend on pyasl, and the C ABI exports of the device implementation."""
import numpy as np
import pytest

import common  # noqa: F401
import rotbroad_numpy as rb


def spectrum(n, lo, dwl, seed):
    rng = np.random.default_rng(seed)
    wl = lo + dwl * np.arange(n)
    flux = 1.0 - 0.4 * rng.random(n) ** 8
    return wl, flux


@pytest.mark.parametrize('n,lo,dwl,vsini,limb', [
    (300, 5000.0, 0.2, 60.0, 0.6),
    (257, 3000.0, 0.2, 150.0, 1.0),
    (64, 7000.0, 0.2, 400.0, 0.05),     # binnu = 47: the halo is most of the extended array
    (40, 30000.0, 0.2, 1000.0, 0.6),    # binnu = 501 >= n
    (50, 7000.0, 0.2, 2.0, 0.6),        # dlmax < dwl
])
def test_literal_and_windowed_forms_agree(n, lo, dwl, vsini, limb):
    wl, flux = spectrum(n, lo, dwl, seed=n)
    a = rb.rot_broad_literal(wl, flux, limb, vsini)
    b = rb.rot_broad(wl, flux, limb, vsini)
    assert np.max(np.abs(a - b) / np.abs(a)) <= 1e-13


@pytest.mark.parametrize('vsini,limb', [(10.0, 0.6), (150.0, 1.0), (1000.0, 0.05)])
def test_constant_spectrum_stays_constant(vsini, limb):
    wl = 7000.0 + 0.2 * np.arange(2000)
    out = rb.rot_broad(wl, np.full(wl.size, 0.73), limb, vsini)
    assert np.max(np.abs(out / 0.73 - 1.0)) <= 1e-15


@pytest.mark.parametrize('eps', [1e-12, 0.6, 1.0])
def test_single_pixel_line_gives_the_gray_profile(eps):
    # dwl = 0.002 A against dlmax = 1.67 A: the discrete profile's normalisation is the integral's to ~1e-5
    dwl, n, p = 0.002, 4001, 2000
    wl = 5000.0 + dwl * np.arange(n)
    flux = np.zeros(n)
    flux[p] = 1.0
    vsini = 100.0
    out = rb.rot_broad(wl, flux, eps, vsini)
    dlmax = vsini / rb.C_KMS * wl
    want = np.array([rb.gray_profile(wl[i] - wl[p], dlmax[i], eps) for i in range(n)]) * dwl
    assert want.max() > 0 and np.max(np.abs(out - want)) <= 1e-3 * want.max()


@pytest.mark.parametrize('vsini,limb', [(30.0, 0.6), (150.0, 0.2), (400.0, 1.0)])
def test_equivalent_width_is_conserved(vsini, limb):
    wl = 6000.0 + 0.05 * np.arange(20000)
    depth = 0.5 * np.exp(-0.5 * ((wl - 6500.0) / 0.4) ** 2)
    out = rb.rot_broad(wl, 1.0 - depth, limb, vsini)
    ew0, ew1 = np.sum(depth) * 0.05, np.sum(1.0 - out) * 0.05
    assert abs(ew1 / ew0 - 1.0) <= 1e-3
    assert np.min(out) > np.min(1.0 - depth)  # and the line did get wider


def test_narrow_profile_is_the_identity():
    wl, flux = spectrum(500, 7000.0, 0.2, seed=3)
    out = rb.rot_broad(wl, flux, 0.6, 5.0)  # dlmax = 0.117 A < dwl
    assert np.max(np.abs(out / flux - 1.0)) <= 2.3e-16


@pytest.mark.parametrize('vsini,limb', [(0.0, 0.5), (-5.0, 0.5), (50.0, 1.5), (50.0, -0.1), (np.nan, 0.5),
                                        (np.inf, 0.5), (50.0, np.nan)])
def test_restatement_refuses_bad_values(vsini, limb):
    wl, flux = spectrum(32, 7000.0, 0.2, seed=1)
    with pytest.raises(ValueError):
        rb.rot_broad(wl, flux, limb, vsini)


def test_library_exports_the_rotation_entries():
    import __graft_entry__ as ge
    from mcmc_spec_amd import _lib
    ge.build()
    lib = _lib.load()
    for name in ('msx_rot_broaden', 'msx_rot_broaden_grid'):
        assert hasattr(lib, name) and name in _lib.EXPORTED
