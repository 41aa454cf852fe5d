"""CPU: the NumPy twin of the derived posteriors (tests/products_numpy.py) against the reference's own
make_composite(plot=True) run (tests/golden/golden_products.npz), the staged band weights against the reference's
integrals on a node row, and the files ``products.reference_files`` writes.  Bar for the goldens: 1e-9 (README)."""
import os

import numpy as np
import pytest
from scipy.interpolate import interp1d

import common
import products_numpy as pn
from common import golden_case
from mcmc_spec_amd import bands, products, staging


@pytest.fixture(scope='module')
def g():
    return dict(np.load(pn.GOLDEN))


def test_golden_file_is_small_and_complete(g):
    assert os.path.getsize(pn.GOLDEN) < os.path.getsize(common.GOLDEN)
    assert g['bin_theta'].shape == (12, 6) and g['nod_theta'].shape == (6, 6) and g['tri_theta'].shape == (6, 8)
    assert g['bin_mags'].shape == (12, 5) and g['tri_mags'].shape == (6, 3, 6)
    assert g['specB'].shape == (3, 4, 700) and g['specA'].shape == (1, 4, 4154)
    th = g['bin_theta']
    assert th[1, 0] == 3800.0 and th[2, 2] == 0.0 and th[3, 0] == 3400.0 and tuple(th[4, :2]) == (3000.0, 4200.0)
    assert g['bin_logg'][2, 1] == 5.0 and g['bin_logg'][3, 0] == 5.0   # on-node log g; (3400, 5.0): both on-node


def test_twin_agrees_with_every_array_of_the_goldens(g):
    worst = pn.check_against(g, tol=1e-9)
    print('worst difference {:.3e}'.format(worst))


def test_staged_weights_reproduce_the_reference_integrals_on_a_node_row(g):
    """TRAPZ, SUM and MEAN weights on grid samples against np.trapz / np.sum / get_flux on the plot=True window of a node
    row: 1e-12 relative (the same products summed in another order)."""
    from oracle import mft6_oracle as orc
    for which in ('A', 'B'):
        c = golden_case(which)
        gb = bands.Band('Gaia_G', g['gaia_wl'], g['gaia_tm'], float(g['gaia_zero_flux'][0]))
        kep = (g['kepler_wl'], g['kepler_tm'])
        pt = staging.build_products(c.wl, c.r, c.tmi, c.tma, c.ctm, c.ptm, pn.products_matrix(), kep, gb,
                                    extra=[('sum', kep)])
        j0, n = pt.window
        reg = staging.product_window_um(c.r, c.tmi, c.tma, c.ctm, c.ptm, g['kepler_wl'])
        w = c.wl[j0:j0 + n]
        lim = np.array(reg) * 1e4
        assert np.array_equal(w, c.wl[np.where((c.wl >= min(lim)) & (c.wl <= max(lim)))])   # mft6.py:537-542
        assert j0 == 0 and w[0] > min(g['kepler_wl'])   # the Kepler curve starts below the grid: its support is clipped
        row = c.flux[7, 2]
        mask = np.where((w >= min(kep[0])) & (w <= max(kep[0])))
        data_tm = interp1d(*kep)(w[mask])
        want = [np.trapz(row[j0:j0 + n][mask] * data_tm, w[mask]),
                orc.OracleBand(g['gaia_wl'], g['gaia_tm']).get_flux(w, row[j0:j0 + n]),
                np.sum(row[j0:j0 + n][mask] * data_tm)]
        assert pt.band_kinds == ['trapz', 'mean', 'sum'] and pt.prod.nbands == 3
        for b, (i0, wts) in enumerate(pt.band_tables):
            got = np.sum(wts * row[i0:i0 + len(wts)])
            assert abs(got - want[b]) <= 1e-12 * abs(want[b]), (which, b, got, want[b])
        assert pt.zero_mag[1] == -2.5 * np.log10(gb.zero_flux) and pt.zero_mag[0] == 0.0


def test_product_isochrone_is_the_first_200_rows(g):
    m = pn.products_matrix()
    t, ma, lu = staging.product_isochrone(m)
    sel = np.where(m[:, 1] == 9.0)[0][:200]
    assert len(t) == 200 and np.all(np.diff(t) >= 0)
    assert np.array_equal(t, np.sort(m[sel, 4])) and t[-1] < staging.sorted_isochrone(m)[0][-1]
    for x in (3001.5, 3400.0, 4199.0):
        assert np.interp(x, t, ma) == pytest.approx(float(interp1d(m[sel, 4], m[sel, 3])(x)), rel=1e-14)
    tl, _, ll = staging.product_isochrone(np.where(np.arange(8)[None, :] == 4, np.log10(np.maximum(m, 1e-30)), m), log_columns=True)
    assert np.allclose(tl, t, rtol=1e-13)


def test_column_names():
    from mcmc_spec_amd import _lib
    codes = products.columns(products.REFERENCE_COLUMNS)
    assert codes[0] == _lib.pcol_dmag(0, 1) and codes[3] == _lib.pcol_bandmag(1, 0) and codes[-1] == _lib.pcol_lum(1)
    assert products.names_of(codes) == list(products.REFERENCE_COLUMNS)
    assert products.columns(['contrast:1', 'phot:5', 'coord:2', 7]) == [_lib.pcol_contrast(1), _lib.pcol_phot(5), 2, 7]
    assert products.columns('kep_sum', bands={'kepler': 3}) == [_lib.pcol_bandmag_sum(3)]
    for bad in ('kepler', 'mass', 'mass:x', 'kep_pri:1'):
        with pytest.raises(ValueError):
            products.columns([bad])


def test_reference_files_are_what_savetxt_writes(g, tmp_path):
    kc, ratio = g['bin_dkep'], g['bin_theta'][:, 4]
    vals = {'kep_contrast': kc, 'gaia_pri': g['bin_mags'][:, 2], 'gaia_sec': g['bin_mags'][:, 3],
            'primary_mass_posterior': g['bin_mass'][:, 0], 'secondary_mass_posterior': g['bin_mass'][:, 1],
            'primary_lum_posterior': g['bin_lum'][:, 0], 'secondary_lum_posterior': g['bin_lum'][:, 1]}
    paths = products.reference_files(str(tmp_path / 'run'), vals, ratio=ratio)
    assert sorted(os.path.basename(p) for p in paths) == sorted(
        ['kep_contrast.txt', 'pri_corr.txt', 'sec_corr.txt', 'gaia_pri.txt', 'gaia_sec.txt', 'primary_mass_posterior.txt',
         'secondary_mass_posterior.txt', 'primary_lum_posterior.txt', 'secondary_lum_posterior.txt'])
    want = dict(vals, pri_corr=g['bin_pri_corr'], sec_corr=g['bin_sec_corr'])   # mft6.py:2544-2545 on the same contrasts
    for p in paths:
        name = os.path.basename(p)[:-4]
        ref = tmp_path / (name + '.ref')
        np.savetxt(str(ref), np.array(want[name]))
        assert open(p).read() == open(str(ref)).read(), name
    with pytest.raises(ValueError):
        products.reference_files(str(tmp_path / 'run'), {'kepler': kc})
