"""NumPy restatement of the rotational broadening the library commits to (DESIGN.md "Rotational broadening"):
PyAstronomy's published ``pyasl.rotBroad(wl, flux, epsilon, vsini, edgeHandling="firstlast")``, with the profile
normalised per output pixel (``out[i] = sum_j f_j g_j / sum_j g_j``).  Parity with pyasl itself is unpinned: it is not
installed here and the reference ships no vectors for it.

Two forms: ``rot_broad_literal`` loops over the whole extended array for every pixel, as pyasl does (O(n^2), small
cases only); ``rot_broad`` is the same arithmetic over each pixel's window of 2 binnu + 1 taps, vectorised."""
import numpy as np

C_KMS = 299792.458


def check(vsini, limb):
    if not (np.isfinite(vsini) and np.isfinite(limb)):
        raise ValueError('vsini and limb must be finite')
    if vsini <= 0.0:
        raise ValueError('vsini must be positive.')
    if limb < 0.0 or limb > 1.0:
        raise ValueError("Linear limb-darkening coefficient, epsilon, should be '0 < epsilon < 1'.")


def extend(wl, flux, vsini):
    """(wl_ext, f_ext, binnu, vc): the slice extended by binnu samples of its first / last value on each side."""
    wl = np.asarray(wl, dtype=float)
    flux = np.asarray(flux, dtype=float)
    dwl = wl[1] - wl[0]
    vc = vsini / C_KMS
    binnu = int(np.floor((vc * max(wl)) / dwl)) + 1
    m = np.arange(binnu) + 1
    wl_ext = np.concatenate(((wl[0] - m * dwl)[::-1], wl, wl[-1] + m * dwl))
    f_ext = np.concatenate((np.ones(binnu) * flux[0], flux, np.ones(binnu) * flux[-1]))
    return wl_ext, f_ext, binnu, vc


def profile(dl, dlmax, eps):
    """Gray's rotation profile g(dl) (zero where |dl / dlmax| >= 1); dlmax may broadcast against dl."""
    c1 = 2. * (1. - eps) / (np.pi * dlmax * (1. - eps / 3.))
    c2 = eps / (2. * dlmax * (1. - eps / 3.))
    x = dl / dlmax
    inside = np.abs(x) < 1.0
    t = np.where(inside, 1. - x**2, 0.0)
    return np.where(inside, c1 * np.sqrt(t) + c2 * t, 0.0)


def rot_broad_literal(wl, flux, limb, vsini):
    check(vsini, limb)
    wl = np.asarray(wl, dtype=float)
    wl_ext, f_ext, binnu, vc = extend(wl, flux, vsini)
    out = np.empty(len(wl))
    for i in range(len(wl)):
        dlmax = vc * wl[i]
        g = profile(wl[i] - wl_ext, dlmax, float(limb))
        out[i] = np.sum(f_ext * g) / np.sum(g)
    return out


def rot_broad(wl, flux, limb, vsini):
    check(vsini, limb)
    wl = np.asarray(wl, dtype=float)
    wl_ext, f_ext, binnu, vc = extend(wl, flux, vsini)
    n = len(wl)
    k = np.arange(2 * binnu + 1)
    out = np.empty(n)
    chunk = max(1, 4000000 // len(k))
    for a in range(0, n, chunk):
        i = np.arange(a, min(n, a + chunk))
        j = i[:, None] + k[None, :]  # pixel i sits at extended index i + binnu
        g = profile(wl[i][:, None] - wl_ext[j], vc * wl[i][:, None], float(limb))
        out[i] = np.sum(f_ext[j] * g, axis=1) / np.sum(g, axis=1)
    return out


def gray_profile(dl, dlmax, eps):
    """The analytic profile G(dl) of a linearly limb-darkened rotating star (unit integral over dl)."""
    x = np.asarray(dl, dtype=float) / dlmax
    t = np.clip(1.0 - x * x, 0.0, None)
    return (2.0 * (1.0 - eps) * np.sqrt(t) + 0.5 * np.pi * eps * t) / (np.pi * dlmax * (1.0 - eps / 3.0))
