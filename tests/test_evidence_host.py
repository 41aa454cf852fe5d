"""CPU: the evidence of a ladder (mcmc_spec_amd.tempered: mean_log_like, log_evidence) -- the formulas
written out, the block partition, the NumPy twin of msx_series_evidence against an independent reference, and the host
sampler against a likelihood whose <ln L>_beta is known."""
import math

import numpy as np
import pytest

import common  # noqa: F401
import evidence_numpy as en
from mcmc_spec_amd import tempered


def hand_made(ll, betas):
    """A host ladder whose stored ln L is ``ll`` (n, T, nw); nothing is sampled."""
    n, T, nw = ll.shape
    s = tempered.TemperedSampler(nw, 2, lambda q: np.zeros(len(q)), lambda q: np.zeros(len(q)), betas=betas, seed=1)
    s._ll = list(ll)
    s._chain = list(np.zeros((n, T, nw, 2)))
    return s


def test_log_evidence_is_the_formulas_written_out():
    rng = np.random.default_rng(3)
    betas = np.array([1.0, 0.5, 0.2, 0.1, 0.04])
    ll = -np.abs(rng.normal(0, 1, (30, 5, 4))) * 3.0 / betas[None, :, None] - 100.0
    s = hand_made(ll, betas)
    m = np.array([np.mean(ll[:, t]) for t in range(5)])
    assert np.array_equal(s.mean_log_like(), m)
    want = ((1.0 - 0.5) * (m[0] + m[1]) / 2 + (0.5 - 0.2) * (m[1] + m[2]) / 2 + (0.2 - 0.1) * (m[2] + m[3]) / 2
            + (0.1 - 0.04) * (m[3] + m[4]) / 2 + 0.04 * m[4])
    coarse = (1.0 - 0.2) * (m[0] + m[2]) / 2 + (0.2 - 0.04) * (m[2] + m[4]) / 2 + 0.04 * m[4]   # rungs 0, 2, 4
    ev = s.log_evidence(blocks=3)
    assert type(ev).__name__ == 'LogEvidence' and ev._fields == ('log_z', 'mc_error', 'ladder_error', 'mean_log_like')
    assert ev.log_z == pytest.approx(want, rel=1e-14) and ev.ladder_error == pytest.approx(abs(want - coarse), rel=1e-12)
    assert np.array_equal(ev.mean_log_like, m)
    per = []
    for b in range(3):   # blocks of 10 rows
        mb = np.array([np.mean(ll[10 * b:10 * b + 10, t]) for t in range(5)])
        per.append(sum((betas[p] - betas[p + 1]) * (mb[p] + mb[p + 1]) / 2 for p in range(4)) + betas[4] * mb[4])
    assert ev.mc_error == pytest.approx(math.sqrt(np.var(per, ddof=1) / 3), rel=1e-10)
    # the stepping stone
    def lme(x, d):
        return math.log(np.mean(np.exp(d * (x - x.max())))) + d * x.max()
    ss = sum(lme(ll[:, t].ravel(), betas[t - 1] - betas[t]) for t in range(1, 5)) + 0.04 * m[4]
    ss_coarse = lme(ll[:, 2].ravel(), 1.0 - 0.2) + lme(ll[:, 4].ravel(), 0.2 - 0.04) + 0.04 * m[4]
    ev = s.log_evidence(blocks=3, method='ss')
    assert ev.log_z == pytest.approx(ss, rel=1e-13) and ev.ladder_error == pytest.approx(abs(ss - ss_coarse), rel=1e-11)
    # an even ladder keeps its last rung: rungs 0, 2, 3 of four; one and two rungs have nothing to drop
    assert tempered.halved(4) == [0, 2, 3] and tempered.halved(5) == [0, 2, 4] and tempered.halved(2) == [0, 1] and tempered.halved(1) == [0]
    s4 = hand_made(ll[:, :4], betas[:4])
    c4 = (1.0 - 0.2) * (m[0] + m[2]) / 2 + (0.2 - 0.1) * (m[2] + m[3]) / 2 + 0.1 * m[3]
    e4 = s4.log_evidence(blocks=1)
    assert e4.ladder_error == pytest.approx(abs(e4.log_z - c4), rel=1e-12) and math.isnan(e4.mc_error)
    s1 = hand_made(ll[:, :1], betas[:1])
    assert s1.log_evidence(blocks=2).log_z == pytest.approx(m[0], rel=1e-15) and s1.log_evidence().ladder_error == 0.0
    # discard / thin select rows[discard::thin]
    assert np.array_equal(s.mean_log_like(discard=4, thin=3), [np.mean(ll[4::3, t]) for t in range(5)])
    for bad in (dict(method='x'), dict(blocks=0), dict(blocks=31), dict(blocks=65), dict(discard=30)):
        with pytest.raises(ValueError):
            s.log_evidence(**bad)


@pytest.mark.parametrize('n,B', [(10, 3), (257, 8), (7, 1), (7, 7), (64, 64), (1000, 64), (5, 4)])
def test_the_blocks_cover_the_rows_once_each(n, B):
    for lo in (en.bounds(n, B), tempered.block_bounds(n, B)):
        assert lo[0] == 0 and lo[-1] == n and len(lo) == B + 1
        sizes = np.diff(lo)
        assert np.all(sizes >= 1) and sizes.sum() == n and sizes.max() - sizes.min() <= 1
        assert sorted(i for b in range(B) for i in range(lo[b], lo[b + 1])) == list(range(n))
    assert en.bounds(n, B) == tempered.block_bounds(n, B)


def inputs(kind, n, counts, rng):
    nw = sum(counts)
    x = rng.normal(-300.0, 40.0, (n, nw))
    if kind == 'equal':
        x[:] = -1234.5678
    elif kind == 'one_inf':
        x[n // 2, 1] = -np.inf
    elif kind == 'all_inf':
        x[:, counts[0]:counts[0] + counts[1]] = -np.inf
    return x


@pytest.mark.parametrize('kind', ['random', 'equal', 'one_inf', 'all_inf'])
def test_the_twin_agrees_with_the_independent_reference(kind):
    rng = np.random.default_rng(11)
    counts, db = [5, 8, 64], np.array([0.0, 0.3, 0.05])
    for n, B in ((1, 1), (300, 7), (513, 2)):
        x = inputs(kind, n, counts, rng)
        got, want = en.twin(x, counts, db, B), en.reference(x, counts, db, B)
        assert en.close(got[0], want[0], 1e-9) and en.close(got[1], want[1], 1e-9), (n, B)
        assert not np.any(np.isnan(got[0])) and not np.any(np.isnan(got[1]))
        if kind == 'all_inf':
            assert np.all(got[0][1] == -np.inf) and np.all(got[1][1] == -np.inf) and np.all(np.isfinite(got[1][2]))
        if kind == 'one_inf':
            assert got[0][0, 0] == -np.inf and np.isfinite(got[1][0, 0]) and np.isfinite(got[0][2, 0])
        host = tempered.host_evidence(x.reshape(n, 1, -1)[:, :, :5], db[:1], B)   # the library's host path, member 0
        assert en.close(host[0], want[0][:1], 1e-9) and en.close(host[1], want[1][:1], 1e-9)
    x = inputs('random', 40, counts, rng)
    x[7, 70] = np.nan
    got = en.twin(x, counts, db, 4)
    assert np.isnan(got[0][2, 0]) and np.isnan(got[1][2, 0]) and np.isnan(got[0][2, 1]) and np.isfinite(got[0][2, 2])
    assert np.all(np.isfinite(got[0][:2])) and np.all(np.isfinite(got[1][:2]))


# ---- the host sampler against a known <ln L>_beta ----------------------------------------------------------------------
D, NW, BETAS = 2, 16, np.geomspace(1.0, 0.05, 5)
HALF = 32.0          # the box's half-width: 7 / sqrt(0.05) = 31.3
BURN, KEEP = 300, 1500


def gaussian_run(seed):
    """ln L = -|x|^2 / 2 inside a flat box: <ln L>_beta = -d / (2 beta) (the box cuts 7 sigma of the hottest rung)."""
    def loglike(q):
        return -0.5 * np.sum(q * q, axis=1)

    def logprior(q):
        return np.where(np.all(np.abs(q) <= HALF, axis=1), 0.0, -np.inf)

    s = tempered.TemperedSampler(NW, D, loglike, logprior, betas=BETAS, seed=seed)
    rng = np.random.default_rng(1000 + seed)
    p0 = rng.normal(0.0, 1.0, (len(BETAS), NW, D)) / np.sqrt(BETAS)[:, None, None]
    st = s.run_mcmc(p0, BURN)
    s.reset()
    s.run_mcmc(st, KEEP)
    return s


def deviations(s):
    exact = -D / (2.0 * BETAS)
    ev = s.log_evidence(blocks=8)
    return float(np.max(np.abs(ev.mean_log_like - exact) / np.abs(exact))), abs(ev.log_z - tempered.ti_log_z(BETAS, exact)), ev


# The bounds: the widest deviation over seeds 1..10 of this host sampler (deviations(gaussian_run(seed))) from the
# analytic values, times 1.5 -- as DESIGN.md section 17 took its swap fractions.
REL_BOUND = 1.5 * 0.02234
LNZ_BOUND = 1.5 * 0.04062


def test_the_host_ladder_recovers_the_analytic_curve():
    """d = 2, 16 walkers, five rungs from 1 to 0.05, 300 + 1500 iterations; seed 11, not one of the ten the bounds come from.

    Seeds 1..10, max_t |m_t - exact_t| / |exact_t|:  0.01406 0.02234 0.01160 0.01077 0.01784 0.02076 0.01549 0.02009 0.01821
    0.01098; |ln Z_ti - trapezoid of the exact curve| (-4.28374):  0.01108 0.01841 0.01151 0.00863 0.02278 0.02172 0.02038
    0.03289 0.04062 0.02408.  (Seed 11: 0.01458 and 0.01824; mc_error 0.065, ladder_error 0.975.)"""
    rel, dz, ev = deviations(gaussian_run(11))
    print('max relative deviation of the rung means', rel, ' |ln Z - exact trapezoid|', dz, ' mc_error', ev.mc_error, ' ladder', ev.ladder_error)
    assert rel <= REL_BOUND and dz <= LNZ_BOUND
    # ladder_error is its definition on the run's own means (five rungs are coarse for a curve like -1 / beta: dropping
    # every other rung moves ln Z by far more than the noise, which is what the figure is there to say)
    half, m = tempered.halved(len(BETAS)), ev.mean_log_like
    assert ev.ladder_error == pytest.approx(abs(tempered.ti_log_z(BETAS, m) - tempered.ti_log_z(BETAS[half], m[half])), rel=1e-12)
    assert ev.mc_error > 0.0
