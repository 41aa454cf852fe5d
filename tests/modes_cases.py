"""Seeded chains for the tests of mcmc_spec_amd.modes, drawn directly from known mixtures: no sampler
runs.  Every chain is (rows, walkers, 6); ``repeat`` of its rows repeat the walker's previous row, as a chain's rejected
proposals do."""
import numpy as np

# the fit's units: Teff1, Teff2 [K], Av [mag], R1, R2/R1, parallax [arcsec]
CENTER = np.array([3850.0, 3400.0, 0.30, 0.45, 0.80, 2.0e-3])
WIDTH = np.array([100.0, 80.0, 0.05, 0.02, 0.04, 2.0e-5])


def _repeat(x, rng, repeat):
    rep = rng.random(x.shape[:2]) < repeat
    rep[0] = False
    for t in range(1, x.shape[0]):
        x[t][rep[t]] = x[t - 1][rep[t]]
    return x


def two_mode(n, W, seed, heavy=0.8, repeat=0.3):
    """Samples of ``test_moves_host.bimodal``'s two unit Gaussians (x0 = -5 with weight ``heavy``, x0 = +5)."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, W, 6))
    x[:, :, 0] += np.where(rng.random((n, W)) < heavy, -5.0, 5.0)
    return _repeat(x, rng, repeat)


def scaled(n, W, seed, heavy=0.8, repeat=0.3):
    """(chain in the fit's units, in_light_mode (n, W)): ``two_mode`` whose light mode has another shape (widths, a
    correlation, a shift in two more columns), mapped by x -> CENTER + WIDTH x."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, W, 6))
    light = rng.random((n, W)) >= heavy
    y = x * np.array([0.5, 1.5, 0.7, 1.2, 0.8, 1.0])
    y[:, :, 2] += 0.6 * y[:, :, 1]
    y += np.array([5.0, 3.0, 0.0, -3.0, 0.0, 0.0])
    x[:, :, 0] -= 5.0
    x[light] = y[light]
    # (the repeats come before the map, on both arrays alike)
    rep = rng.random((n, W)) < repeat
    rep[0] = False
    for t in range(1, n):
        x[t][rep[t]] = x[t - 1][rep[t]]
        light[t][rep[t]] = light[t - 1][rep[t]]
    return CENTER + WIDTH * x, light


def one_gauss(n, W, seed, repeat=0.3):
    """One correlated Gaussian in the fit's units."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(n, W, 6))
    x[:, :, 1] += 0.5 * x[:, :, 0]
    x[:, :, 4] -= 0.3 * x[:, :, 3]
    return CENTER + WIDTH * _repeat(x, rng, repeat)
