"""``Engine``: one GPU, one staged model grid, one staged dataset -- the object the drop-in functions
in ``mcmc_spec_amd.mft6`` cache behind the reference's call signatures.

All numerics run in ``libmsx.so`` (HIP, gfx950).  This class only moves arguments across the C ABI
and maps per-walker status codes onto the exceptions the reference would raise.
"""
from __future__ import annotations

import numpy as np

from . import _lib
from . import staging


def _raise_for_status(status, theta):
    bad = np.nonzero(status > _lib.W_REJECT)[0]
    if bad.size == 0:
        return
    i = int(bad[0])
    code = int(status[i])
    where = 'walker {} (theta = {})'.format(i, np.array2string(np.asarray(theta)[i], precision=6))
    if code == _lib.W_KEYERROR:
        raise KeyError('a model grid node needed by {} is not in specs'.format(where))  # mft6.py:489-500
    if code == _lib.W_INDEXERROR:
        raise IndexError('list index out of range: Teff/logg bracket past the last grid node for ' + where)
    if code == _lib.W_VALUEERROR:
        raise ValueError('A value in x_new is outside the interpolation range (isochrone Teff) for ' + where)
    if code == _lib.W_HANDOVER:
        raise RuntimeError('device fault: workgroups that wait for each other inside a launch (the linked form; the '
                           'overlapped half-steps of the device-resident sampler) did not meet within 20 ms for ' + where +
                           ' (stage the problem again before the next launch)')
    raise RuntimeError('unknown walker status {} for {}'.format(code, where))


def component_rotations(vsini, limb):
    """``None`` for scalar ``vsini`` and ``limb`` (one rotation for the whole grid); else the list of per-star
    ``(vsini, limb)`` pairs, 1..3 of them (a scalar beside a sequence is repeated).  ValueError on unequal lengths."""
    seq_v, seq_l = np.ndim(vsini) > 0, np.ndim(limb) > 0
    if not seq_v and not seq_l:
        return None
    v = [float(x) for x in np.ravel(vsini)] if seq_v else None
    lb = [float(x) for x in np.ravel(limb)] if seq_l else None
    n = len(v) if v is not None else len(lb)
    v = v if v is not None else [float(vsini)] * n
    lb = lb if lb is not None else [float(limb)] * n
    if len(v) != len(lb):
        raise ValueError('vsini and limb: one value per star each ({} and {} given)'.format(len(v), len(lb)))
    if not 1 <= n <= _lib.MAX_SPEC:
        raise ValueError('vsini / limb per star: 1 to {} stars, {} given'.format(_lib.MAX_SPEC, n))
    return list(zip(v, lb))


class Engine:
    def __init__(self, device=0):
        self.ctx = _lib.Context(device)
        self.device = device
        self.grid = None
        self.tables = None
        self.products = None

    # ---- A0 ---------------------------------------------------------------------------------------
    def stage_grid(self, wl, teff_nodes, logg_nodes, flux, present=None):
        self.ctx.stage_grid(wl, teff_nodes, logg_nodes, flux, present)
        self._grid_meta(wl, teff_nodes, logg_nodes)

    def stage_specs(self, specs):
        """``specs``: the reference's dict, or a tuple of ``nspec`` such dicts -- one per star, sharing keys and ``wl``
        (``parse_component_specs``) -- staged as a component grid (copy s for star s)."""
        if isinstance(specs, (tuple, list)):
            teff, logg, wl, flux, present = staging.parse_component_specs(specs)
            self.ctx.stage_grid_components(wl, teff, logg, flux, present)
            self._grid_meta(wl, teff, logg)
            return
        teff, logg, wl, flux, present = staging.parse_specs(specs)
        self.stage_grid(wl, teff, logg, flux, present)

    def _grid_meta(self, wl, teff_nodes, logg_nodes):
        self.grid = dict(wl=np.asarray(wl, dtype=float), teff=np.asarray(teff_nodes, dtype=float),
                         logg=np.asarray(logg_nodes, dtype=float))
        self.tables = None
        self.products = None

    def broaden_grid_window(self, w_aa, resolution, placement='staging', vsini=0, limb=0):
        """Broaden every node over the data window ``[min(w), max(w)]`` [A] in place: the staging step
        of ``spec_interpolator`` (mft6.py:366-378).  ``placement='in_path'`` additionally keeps the raw window on the
        device: problems staged afterwards can be evaluated with the broadening applied per walker
        (``ctx.set_path(_lib.PATH_INPATH)``) beside the default forms.

        ``vsini`` [km/s] / ``limb``: when both are nonzero (the reference's condition, mft6.py:133), the same window is
        then rotationally broadened (``pyasl.rotBroad``; ValueError on a bad value).  A rotated grid has no in-path form.

        Per star (an extension of the reference's signature): ``vsini`` and ``limb`` may be sequences of one value per
        star (a scalar beside a sequence is repeated).  The grid is then split after the Gaussian into a component
        grid of ``ncomp`` copies (DESIGN.md "Component grids"), and copy s is rotated with ``(vsini[s], limb[s])`` under
        the same condition; a copy whose pair fails it stays Gaussian-only.  Problems staged on it need
        ``nspec == ncomp``."""
        pairs = component_rotations(vsini, limb)
        self.ctx.set_broadening(placement)
        wl = self.grid['wl']
        idx = np.where((wl >= min(w_aa)) & (wl <= max(w_aa)))[0]
        self.ctx.broaden_grid(int(idx[0]), int(idx.size), resolution, 5.0)
        self.tables = None
        self.products = None   # (the library drops the problem and its products with it)
        if pairs is None:
            if vsini != 0 and limb != 0:
                self.ctx.rot_broaden_grid(int(idx[0]), int(idx.size), vsini, limb)
            return
        self.ctx.split_components(len(pairs))
        for s, (vs, ls) in enumerate(pairs):
            if vs != 0 and ls != 0:
                self.ctx.rot_broaden_grid_component(s, int(idx[0]), int(idx.size), vs, ls)

    # ---- problem ------------------------------------------------------------------------------------
    def stage_problem(self, data, err, fr, r, ctm, ptm, tmi, tma, matrix, nspec=2, bands=None, av_table=None,
                      tmin=-np.inf, tmax=np.inf, prior=0, use_av=True, dist_fit=True, rad_prior=False, spectrum=True,
                      store='f64'):
        """``store='f32'`` keeps the per-node pixel table R in float32 (include/msx.h, msx_set_grid_storage): a SEPARATELY
        LABELLED storage precision -- ~1e-7 relative on the log-probability at S/N 100 instead of the float64 tables'
        1e-13, a quarter fewer bytes through the CU's L2 port; fused binaries only.  Default: float64."""
        if self.grid is None:
            raise RuntimeError('stage the model grid first')
        self.ctx.set_grid_storage(store)
        st = staging.build_problem(self.ctx, self.grid['wl'], data, err, fr, r, ctm, ptm, tmi, tma, matrix,
                                   nspec=nspec, bands=bands, av_table=av_table, tmin=tmin, tmax=tmax, prior=prior,
                                   use_av=use_av, dist_fit=dist_fit, rad_prior=rad_prior, spectrum=spectrum)
        self.ctx.stage_problem(st.prob)
        self.tables = st
        self._tm = (ctm, ptm)   # (products.stage builds the plot=True window from the same curves)
        self.products = None    # the library drops staged products with the problem
        self.nspec = int(nspec)
        self.ndim = 2 * self.nspec + 2

    # ---- hot path -----------------------------------------------------------------------------------
    def _eval(self, theta, mode):
        theta = np.asarray(theta, dtype=float)
        single = theta.ndim == 1
        th = np.atleast_2d(theta)
        if th.shape[1] != self.ndim:
            raise ValueError("P0 doesn't match what I was expecting")  # mft6.py:1457
        logp, status = self.ctx.logprob_batch(th, mode)
        _raise_for_status(status, th)
        return float(logp[0]) if single else logp

    def logposterior(self, theta):
        return self._eval(theta, _lib.MODE_LOGPOST)

    def logprior(self, theta):
        return self._eval(theta, _lib.MODE_LOGPRIOR)

    def loglikelihood(self, theta, optimize=False):
        return self._eval(theta, _lib.MODE_CHISQ if optimize else _lib.MODE_LOGLIKE)

    def stage_products(self, kepler, gaia=None, matrix=None, **kw):
        """``products.stage`` on this engine: the Kepler / Gaia product bands and the mass-luminosity isochrone."""
        from . import products
        return products.stage(self, kepler, gaia, matrix, **kw)

    def derived(self, theta, cols):
        """``products.evaluate``: the derived columns (names or codes) of the samples ``theta``."""
        from . import products
        return products.evaluate(self, theta, cols)

    def make_composite(self, teff, logg, rad, distance):
        """Returns (wl, spec, contrast list, phot_cwl, phot) like mft6.py:831."""
        st = self.tables
        use_d = not (type(distance) == bool)
        spec, con, ph, status = self.ctx.make_composite(teff, logg, rad, use_d, float(distance) if use_d else 0.0,
                                                        st.window[1], st.nc, st.nph)
        _raise_for_status(np.array([status]), np.array([list(teff) + list(logg)]))
        j0, n = st.window
        return (self.grid['wl'][j0:j0 + n].copy(), spec, [c for c in con], st.phot_cwl.copy(), ph)
