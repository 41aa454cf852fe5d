"""Test-side restatement of the likelihood on a component grid (DESIGN.md "Component grids"): star s of the model is
interpolated from its own ``specs[s]`` -- e.g. a grid rotated with star s's v sin i -- and everything after the
interpolation is the oracle's (oracle/mft6_oracle.py, imported, not modified).

Star s is the 6th return (``stars``) of ``oracle.make_composite`` called with ``specs[s]``; the component sum, the
contrasts and the photometry are then recomputed here exactly as ``make_composite`` computes them, and the rest is the
oracle's ``loglikelihood`` from the reddening on (``extinct``, ``norm_spec``, ``chisq``).  With one ``specs`` for every
star this is ``oracle.loglikelihood`` bit for bit (tests/test_component_restatement.py)."""
import numpy as np
from scipy.interpolate import interp1d

from oracle import mft6_oracle as orc


def make_composite_components(teff, logg, rad, distance, contrast_filt, phot_filt, r, specs_seq, ctm, ptm, tmi, tma,
                              nspec=2, bandlib=None):
    """``oracle.make_composite`` with star s taken from ``specs_seq[s]``: (wave, comp, contrast, phot_cwl, phot, stars)."""
    stars, wave, phot_cwl = [], None, None
    for s in range(len(teff)):
        out = orc.make_composite(teff, logg, rad, distance, contrast_filt, phot_filt, r, specs_seq[s], ctm, ptm, tmi, tma,
                                 nspec=nspec, bandlib=bandlib)
        wave, phot_cwl = out[0], out[3]
        stars.append(out[5][s])
    stars = np.vstack(stars)
    wls, tras = ctm[0], ctm[1]
    mag = np.zeros((len(contrast_filt), len(teff)))
    for n in range(len(contrast_filt)):
        ran, tm = wls[n], tras[n]
        inband = np.where((wave <= max(ran)) & (wave >= min(ran)))
        w = wave[inband]
        tran = interp1d(ran, tm)(w)
        for k in range(len(teff)):
            m = np.trapz(stars[k][inband] * tran, w)
            mag[n][k] = -2.5 * np.log10(m)
    if float(nspec) == 2:
        contrast = [mag[n][1] - mag[n][0] for n in range(len(contrast_filt))]
        comp = stars[0] + stars[1]
    else:
        c1 = [mag[n][1] - mag[n][0] for n in range(len(contrast_filt))]
        c2 = [mag[n][2] - mag[n][0] for n in range(len(contrast_filt))]
        h = int(len(contrast_filt) / 2)
        contrast = list(np.concatenate((c1[:h], c2[h:])))
        comp = stars[0] + stars[1] + stars[2]
    names = orc.PHOT_BANDS_3 if len(phot_filt) == 3 else orc.PHOT_BANDS_6
    phot = []
    for n in range(len(phot_filt)):
        band = bandlib[names[n]]
        f = band.get_flux(wave, comp)
        zero = band.Vega_zero_flux if '2MASS' in names[n] else band.AB_zero_flux
        phot.append(-2.5 * np.log10(f / zero))
    return (np.array(wave), np.array(comp), [c for c in contrast], np.array([float(p) for p in phot_cwl]),
            np.array(phot), stars)


def loglikelihood(p0, fr, nspec, data, err, r, specs_seq, ctm, ptm, tmi, tma, matrix, av=True, optimize=False,
                  bandlib=None):
    """``oracle.loglikelihood`` (no ``parts`` / ``inpath``) on per-star specs."""
    wl, spec = np.array(data)
    t_guess = p0[:nspec]
    a_v = p0[nspec]
    rad = p0[nspec + 1:2 * nspec + 1]
    plx = p0[2 * nspec + 1]
    lg = [orc.get_logg(t, matrix) for t in t_guess]
    wave1, cspec, contrast, phot_cwl, phot, _ = make_composite_components(
        t_guess, lg, rad, plx, fr[2], fr[5], r, specs_seq, ctm, ptm, tmi, tma, nspec=nspec, bandlib=bandlib)
    if av == True and a_v > 0:  # noqa: E712  (the reference's test)
        cspec = orc.extinct(wave1, cspec, a_v)
        init_phot = -2.5 * np.log10(orc.extinct(phot_cwl, 10 ** (-0.4 * phot), a_v))
    else:
        init_phot = phot
    model = interp1d(wave1, cspec)(wl * 1e4)
    model = model * (np.median(spec) / np.median(model))
    spec_n = orc.norm_spec(wl, model, spec)
    ic = orc.chisq(model, spec_n, err)
    iic = np.sum(ic) / len(ic)
    chi_c = orc.chisq(contrast, fr[0], fr[1])
    chi_p = orc.chisq(init_phot, fr[3], fr[4])
    total = np.sum((iic * (len(chi_c) + len(chi_p)), np.sum(chi_c), np.sum(chi_p)))
    if optimize:
        return total
    return -np.inf if np.isnan(total) else -0.5 * total


def logposterior(p0, fr, nspec, data, err, r, specs_seq, ctm, ptm, tmi, tma, tmin, tmax, matrix, av_prior, prior=0,
                 a=True, dist_fit=True, rad_prior=False, bandlib=None):
    """``oracle.logposterior`` on per-star specs (the prior does not read the grid)."""
    lp = orc.logprior(p0, nspec, tmin, tmax, matrix, av_prior, prior=prior, ext=a, dist_fit=dist_fit,
                      rad_prior=rad_prior)
    if not np.isfinite(lp):
        return -np.inf
    return lp + loglikelihood(p0, fr, nspec, data, err, r, specs_seq, ctm, ptm, tmi, tma, matrix, av=a, bandlib=bandlib)
