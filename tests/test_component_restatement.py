"""CPU: the per-star restatement of the likelihood (tests/component_restatement.py) is the oracle's when every star reads
the same specs; the host-side checks of per-star specs and per-star rotations."""
import numpy as np
import pytest

import common
from common import golden_case
import component_restatement as cr


@pytest.mark.parametrize('which', ['B', 'C'])
def test_restatement_is_the_oracle_with_one_specs(which):
    c = golden_case(which)
    seq = (c.specs,) * c.nspec
    for th in c.theta[:6]:
        want = common.oracle_loglike(c, th)
        got = cr.loglikelihood(list(th), c.fr, c.nspec, c.data, c.err, c.r, seq, c.ctm, c.ptm, c.tmi, c.tma, c.matrix,
                               bandlib=c.bandlib)
        assert np.array_equal(got, want, equal_nan=True)
    th = c.theta[0]
    want = common.oracle_logpost(c, th, rad_prior=c.nspec == 3)
    got = cr.logposterior(list(th), c.fr, c.nspec, c.data, c.err, c.r, seq, c.ctm, c.ptm, c.tmi, c.tma, c.tmin, c.tmax,
                          c.matrix, common.av_prior, prior=c.prior, rad_prior=c.nspec == 3, bandlib=c.bandlib)
    assert np.array_equal(got, want, equal_nan=True)


def test_restatement_reads_star_s_from_specs_s():
    """A change to specs[1] alone moves the binary's likelihood; the same change in specs[0] alone does too, and
    differently: each star reads its own dict."""
    c = golden_case('B')
    scaled = {k: (v if k == 'wl' else 1.01 * np.asarray(v)) for k, v in c.specs.items()}
    th = list(c.theta[0])
    args = (c.fr, 2, c.data, c.err, c.r)
    rest = (c.ctm, c.ptm, c.tmi, c.tma, c.matrix)
    base = cr.loglikelihood(th, *args, (c.specs, c.specs), *rest, bandlib=c.bandlib)
    a = cr.loglikelihood(th, *args, (scaled, c.specs), *rest, bandlib=c.bandlib)
    b = cr.loglikelihood(th, *args, (c.specs, scaled), *rest, bandlib=c.bandlib)
    assert len({float(base), float(a), float(b)}) == 3


def test_per_star_specs_must_share_keys_and_axis():
    from mcmc_spec_amd import staging
    c = golden_case('B')
    teff, logg, wl, flux, present = staging.parse_component_specs((c.specs, c.specs))
    assert flux.shape == (2, len(teff), len(logg), len(wl)) and np.array_equal(flux[0], flux[1])
    fewer = dict(c.specs)
    fewer.pop(next(k for k in fewer if k != 'wl'))
    with pytest.raises(ValueError, match='keys'):
        staging.parse_component_specs((c.specs, fewer))
    moved = dict(c.specs)
    moved['wl'] = np.asarray(c.specs['wl']) + 0.1
    with pytest.raises(ValueError, match='wl'):
        staging.parse_component_specs((c.specs, moved))
    with pytest.raises(ValueError, match='1 to 3'):
        staging.parse_component_specs((c.specs,) * 4)
    with pytest.raises(ValueError, match='dict'):
        staging.parse_component_specs((c.specs, 3))


def test_per_star_rotations():
    from mcmc_spec_amd.engine import component_rotations
    assert component_rotations(60, 0.6) is None and component_rotations(0, 0) is None
    assert component_rotations((60, 10), (0.6, 0.3)) == [(60.0, 0.6), (10.0, 0.3)]
    assert component_rotations([60, 0, 5], 0.5) == [(60.0, 0.5), (0.0, 0.5), (5.0, 0.5)]
    assert component_rotations(20, (0.1, 0.2)) == [(20.0, 0.1), (20.0, 0.2)]
    with pytest.raises(ValueError, match='one value per star'):
        component_rotations((60, 10), (0.6, 0.3, 0.2))
    with pytest.raises(ValueError, match='stars'):
        component_rotations((1, 2, 3, 4), 0.5)
    with pytest.raises(ValueError, match='stars'):
        component_rotations((), ())


def test_component_entries_are_exported():
    from mcmc_spec_amd import _lib
    for name in ('msx_split_components', 'msx_stage_grid_components', 'msx_rot_broaden_grid_component',
                 'msx_read_node_component'):
        assert name in _lib.EXPORTED
