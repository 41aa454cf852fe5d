"""High-precision twin of the Gaussian instrumental broadening and the checker the GPU tests hold the two
implementations to: ``broaden_conv_kernel`` / ``broaden_patch_kernel`` (csrc/staging_kernels.h) and ``inpath_conv_kernel``
(csrc/inpath_kernels.h).  CPU only; tests/test_broaden_restatement.py proves the checker on emulations of the kernels
(right and deliberately wrong ones), tests/test_gpu_broaden_shapes.py applies it to the device.

The definition is the kernels' own comment: ``out[i] = sum_k e[k] y[i + c - k]``, ``c = (lx - 1) // 2``, zero outside
``[0, n)``, with PyAstronomy's ``broadGaussFast`` taps ``x_k = (k - off0) dx``, ``off0 = lx // 2 + lx % 2 - 1``.  It always
has ``n`` samples -- also where ``lx > n`` (there ``np.convolve(y, e, 'same')`` returns ``lx`` samples).

The bound of ``check`` is derived, not measured: a recursive float64 sum of ``lx`` terms is off by at most
``lx 2^-53 sum |terms|`` with or without fused multiply-adds; sixteen more units cover a few ulp in each device ``exp`` and
in the normalisation.  It is absolute, so rows that change sign or vanish are held to it like any other."""
import numpy as np

if np.finfo(np.longdouble).eps >= 2.0 ** -60:
    raise ImportError('tests/broaden_numpy.py needs a long double wider than float64 (eps %g here): the reference would be '
                      'no more precise than the kernels it judges' % np.finfo(np.longdouble).eps)

LD = np.longdouble
TILE = 1024          # kConvTile
U = 2.0 ** -53


def off0_of(lx):
    return lx // 2 + lx % 2 - 1


def centre_of(lx):
    return (lx - 1) // 2


def taps(dx, sigma, lx):
    """The kernel's normalised taps in long double."""
    x = (np.arange(lx) - off0_of(lx)).astype(LD) * LD(dx)
    e = np.exp(-(x * x) / (LD(2) * (LD(sigma) * LD(sigma))))
    return e / np.sum(e)


def mean_sequential(wl):
    """mean(wl) as msx_broaden sums it: one float64 accumulator, ascending."""
    return float(np.cumsum(np.asarray(wl, dtype=float))[-1] / float(len(wl)))


def sigma_of(mean_wl, resolution):
    """conv_taps (csrc/msx.hip): fwhm = 1 / R * mean(wl); sigma = fwhm / (2 sqrt(2 ln 2)), float64, same order."""
    fwhm = 1.0 / float(resolution) * float(mean_wl)
    return fwhm / (2.0 * np.sqrt(2.0 * np.log(2.0)))


def lx_of(mean_wl, dx, resolution, maxsig):
    """conv_taps: lx = int(((sigma * maxsig) / dx) * 2.0) + 1."""
    return int(((sigma_of(mean_wl, resolution) * float(maxsig)) / float(dx)) * 2.0) + 1


def lds_bytes(lx):
    """launch_conv's dynamic LDS: the taps and a tile with its halo."""
    return 8 * (lx + TILE + lx - 1)


def inpath_lds_bytes(lx):
    """msx_stage_problem's, for inpath_conv_kernel: the tile padded by one word per four."""
    return 8 * (lx + ((TILE + lx - 1) * 5) // 4 + 2)


def conv_same(y, e):
    """(out, mag): out[i] = sum_k e[k] y[i + c - k], mag[i] = sum_k |e[k] y[i + c - k]|, in long double."""
    y = np.asarray(y).astype(LD)
    e = np.asarray(e).astype(LD)
    n, lx = len(y), len(e)
    c = centre_of(lx)
    # pad[j] = y[j - (lx - 1 - c)]: sample i + c - k sits at pad index i + lx - 1 - k
    pad = np.zeros(n + lx - 1, dtype=LD)
    pad[lx - 1 - c:lx - 1 - c + n] = y
    out, mag = np.zeros(n, dtype=LD), np.zeros(n, dtype=LD)
    for k in range(lx):
        t = e[k] * pad[lx - 1 - k:lx - 1 - k + n]
        out += t
        mag += np.abs(t)
    return out, mag


def patch(b):
    """b[0:5] = b[5]; b[n-10:n] = b[n-11] (mft6.py:129-130), on a copy."""
    b = np.array(b)
    n = len(b)
    b[0:5] = b[5]
    b[n - 10:n] = b[n - 11]
    return b


def check(got, y, dx, sigma, lx, patched):
    """Assert |got[i] - ref[i]| <= (lx + 16) 2^-53 mag[i] for every sample -- a patched sample against its source's
    reference and magnitude -- and, where ``patched``, that the 5 + 10 patched samples carry the bits of got[5] and
    got[n-11].  Returns the worst |got - ref| / bound over the row (0 where both vanish)."""
    got = np.asarray(got, dtype=float)
    n = len(y)
    assert got.shape == (n,), (got.shape, n)
    assert np.all(np.isfinite(got))
    ref, mag = conv_same(y, taps(dx, sigma, lx))
    if patched:
        ref, mag = patch(ref), patch(mag)
        assert np.array_equal(got[0:5], np.full(5, got[5])), 'left patch: not the bits of sample 5'
        assert np.array_equal(got[n - 10:n], np.full(10, got[n - 11])), 'right patch: not the bits of sample n - 11'
    err = np.abs(got.astype(LD) - ref)
    bound = LD(lx + 16) * LD(U) * mag
    bad = np.flatnonzero(err > bound)
    assert bad.size == 0, 'sample %d of %d (lx %d): |got - ref| = %.3e > bound %.3e (%d samples over)' % (
        bad[0], n, lx, float(err[bad[0]]), float(bound[bad[0]]), bad.size)
    ratio = np.where(bound > 0, err / np.where(bound > 0, bound, LD(1)), LD(0))
    return float(ratio.max())


# ---- the axis, the rows and the cases of the GPU tests (tests/test_gpu_broaden_shapes.py) -------------------------------
def axis(n):
    return 7000.0 + 0.2 * np.arange(n)


def rows(n):
    """(wl, y, y - 1): the test row and its sign-changing twin, seeded by n."""
    wl = axis(n)
    y = 1.0 + 0.3 * np.sin(wl / 7.0) + 0.05 * np.random.default_rng(4000 + n).normal(size=n)
    return wl, y, y - 1.0


def params(n, resolution, maxsig):
    """(dx, sigma, lx) of msx_broaden on axis(n)."""
    wl = axis(n)
    m = mean_sequential(wl)
    assert lx_of(m, wl[1] - wl[0], resolution, maxsig) == lx_of(float(np.mean(wl)), wl[1] - wl[0], resolution, maxsig)
    return wl[1] - wl[0], sigma_of(m, resolution), lx_of(m, wl[1] - wl[0], resolution, maxsig)


def pick_resolution(n, accept, start, step=0.999):
    """The first R = start * step^j whose lx on axis(n) (maxsig 5) satisfies accept(lx)."""
    r = float(start)
    for _ in range(20000):
        if accept(params(n, r, 5.0)[2]):
            return r
        r *= step
    raise AssertionError('no resolution found')


MAX_LX = 9088        # 8 (2 lx + 1023) <= 150 KiB
N_LONGEST = 1100


def longest_resolution():
    """The largest kernel launch_conv accepts on axis(N_LONGEST): lx in [8900, 9088]."""
    return pick_resolution(N_LONGEST, lambda lx: 8900 <= lx <= MAX_LX, 17.5)


def refused_resolution():
    return pick_resolution(N_LONGEST, lambda lx: lx > MAX_LX, 17.5)


# (id, n, R, maxsig, what lx must be: a predicate of (lx, n))
CASES = (
    ('identity', 17, 1e6, 5.0, lambda lx, n: lx == 1),
    ('even2', 64, 1e5, 5.0, lambda lx, n: lx == 2),
    ('n16', 16, 1700.0, 5.0, lambda lx, n: lx > n and lx <= 256),
    ('n64', 64, 1700.0, 5.0, lambda lx, n: lx > n and lx <= 256),
    ('n300', 300, 400.0, 5.0, lambda lx, n: lx > n and lx > 256),
    ('n1023', 1023, 1700.0, 5.0, lambda lx, n: lx % 2 == 1 and 1 < lx <= 256),
    ('n1024_even', 1024, 1700.0, 5.06, lambda lx, n: lx % 2 == 0 and 2 < lx <= 256),
    ('n1025_two_trips', 1025, 400.0, 5.0, lambda lx, n: 256 < lx <= 512),
    ('n1027', 1027, 5000.0, 5.0, lambda lx, n: lx % 2 == 1 and 1 < lx <= 256),
    ('n2049_even', 2049, 1700.0, 3.3, lambda lx, n: lx % 2 == 0 and 2 < lx <= 256),
    ('longer_than_tile', 3000, 120.0, 5.0, lambda lx, n: TILE < lx < n and lds_bytes(lx) <= 64 * 1024),
    ('lds_attribute', 1500, 40.0, 5.0, lambda lx, n: lx > n and lds_bytes(lx) > 64 * 1024),
)


def case_params(case):
    """(n, dx, sigma, lx) of a case, its class asserted."""
    cid, n, resolution, maxsig, cls = case
    dx, sigma, lx = params(n, resolution, maxsig)
    assert cls(lx, n), (cid, lx)
    return n, dx, sigma, lx


# ---- float64 emulations of the kernels' summation order (and of four ways to get it wrong) -------------------------------
def taps_f64(dx, sigma, lx, off0=None):
    """The taps as a workgroup of 256 threads builds them: thread t sums taps t, t + 256, ...; a butterfly inside each
    wave of 64; (p0 + p1) + (p2 + p3); one division per tap."""
    off0 = off0_of(lx) if off0 is None else off0
    x = (np.arange(lx) - off0).astype(float) * float(dx)
    e = np.exp(-(x * x) / (2.0 * (float(sigma) * float(sigma))))
    part = np.zeros(256)
    for k0 in range(0, lx, 256):
        seg = e[k0:k0 + 256]
        part[:len(seg)] += seg
    w = part.reshape(4, 64)
    for s in (32, 16, 8, 4, 2, 1):
        w = w[:, :s] + w[:, s:2 * s]
    norm = (w[0, 0] + w[1, 0]) + (w[2, 0] + w[3, 0])
    return e / norm


def emulate(y, dx, sigma, lx, mutant=None):
    """The tiled convolution in float64: per 1,024-sample tile a halo of lx - 1 samples, zero outside the row, every
    output's sum over the taps in ascending order (both kernels; the in-path one stores four adjacent outputs per
    thread behind guards o + j < n).

    mutant: 'centre' (c + 1 for c), 'off0' (the odd formula lx // 2 whatever lx), 'tail' (the last n % 4 outputs of the
    last tile left unwritten), 'halo' (the tile taken from t0 - c instead of t0 - (lx - 1 - c))."""
    y = np.asarray(y, dtype=float)
    n = len(y)
    c = centre_of(lx) + (1 if mutant == 'centre' else 0)
    e = taps_f64(dx, sigma, lx, off0=lx // 2 if mutant == 'off0' else None)
    out = np.zeros(n)
    for t0 in range(0, n, TILE):
        g0 = t0 - c if mutant == 'halo' else t0 + c - (lx - 1)
        g = g0 + np.arange(TILE + lx - 1)
        ok = (g >= 0) & (g < n)
        tile = np.where(ok, y[np.clip(g, 0, n - 1)], 0.0)
        s = np.zeros(TILE)
        for k in range(lx):
            s = s + e[k] * tile[lx - 1 - k:lx - 1 - k + TILE]
        m = min(TILE, n - t0)
        if mutant == 'tail' and t0 + TILE >= n:
            m -= n % 4
        out[t0:t0 + m] = s[:m]
    return out


def composite(rows8, w8):
    """inpath_conv_kernel's composite: star by star, four corners each, then the two stars' sum (float64)."""
    s0, s1 = np.zeros(rows8.shape[1]), np.zeros(rows8.shape[1])
    for k in range(4):
        s0 = s0 + w8[k] * rows8[k]
        s1 = s1 + w8[4 + k] * rows8[4 + k]
    return s0 + s1


# ---- the linear resample of the same loader path (resample_kernel, csrc/staging_kernels.h) -------------------------------
def resample_inputs():
    """(xs, ys, xq): 400 sorted two-decimal abscissae -- 390 distinct knots, four of them twice and three three times --
    and queries on every knot, at both ends and at 1,000 random places."""
    rng = np.random.default_rng(77)
    knots = np.sort(rng.choice(np.arange(500000, 900000), size=390, replace=False)) / 100.0
    twice, thrice = knots[[3, 57, 200, 388]], knots[[0, 120, 389]]
    xs = np.sort(np.concatenate([knots, twice, thrice, thrice]))
    assert len(xs) == 400 and np.all(np.round(xs, 2) == xs)
    ys = 1.0 + rng.normal(size=len(xs))
    xq = np.concatenate([knots, [xs[0], xs[-1]], rng.uniform(xs[0], xs[-1], size=1000)])
    return xs, ys, xq


def resample_numpy(xs, ys, xq):
    """resample_kernel in NumPy: j = the last knot <= x; ys[j] on a knot and at the right end, else
    (ys[j+1] - ys[j]) / (xs[j+1] - xs[j]) * (x - xs[j]) + ys[j] -- np.interp's arithmetic."""
    xs, ys, xq = (np.asarray(a, dtype=float) for a in (xs, ys, xq))
    n = len(xs)
    j = np.searchsorted(xs, xq, side='right') - 1
    jj = np.clip(j, 0, n - 2)
    with np.errstate(divide='ignore', invalid='ignore'):
        slope = (ys[jj + 1] - ys[jj]) / (xs[jj + 1] - xs[jj])
        r = slope * (xq - xs[jj]) + ys[jj]
    r = np.where(xs[np.clip(j, 0, n - 1)] == xq, ys[np.clip(j, 0, n - 1)], r)
    return np.where(j >= n - 1, ys[n - 1], r)
