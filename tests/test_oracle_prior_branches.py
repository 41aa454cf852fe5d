"""CPU: the oracle's logprior / logposterior against the reference on every prior branch (tests/golden/golden_prior.npz,
made by tests/golden/make_prior_golden.py): ndim {6, 8} x dist_fit x ext x rad_prior x prior list, both A_V tables,
random walkers, every gate bound one ulp either side, A_V-table edges and Teffs outside the isochrone."""
import os
import warnings

import numpy as np
import pytest

import common
from common import rel_err
from oracle import mft6_oracle as orc

warnings.filterwarnings('ignore')

PRIOR_GOLDEN = os.path.join(common.ROOT, 'tests', 'golden', 'golden_prior.npz')
OK, NEG_INF, NONE, VALUEERROR, TYPEERROR = 0, 1, 2, 3, 4


def prior_golden():
    return np.load(PRIOR_GOLDEN)


def av_prior_of(g, table):
    """The A_V(distance) prior the reference's stub gave, bin for bin (mean / std of its samples, before 0.05)."""
    edges, mu, sig = g['av%d_edges' % table], g['av%d_mu' % table], g['av%d_sig' % table]

    def av_prior(dist_pc):
        b = int(np.clip(np.searchsorted(edges, dist_pc, side='right') - 1, 0, len(mu) - 1))
        return mu[b], sig[b]
    return av_prior


def outcome(fn):
    try:
        v = fn()
    except ValueError:
        return np.nan, VALUEERROR
    except TypeError:
        return np.nan, TYPEERROR
    if v is None:
        return np.nan, NONE
    v = float(v)
    return (v, NEG_INF) if v == -np.inf else (v, OK)


def oracle_priors(g, ndim, table, combo):
    df, ext, rp, hp = (bool(x) for x in g['combos%d' % ndim][combo])
    ns = (ndim - 2) // 2
    prior = list(g['prior%d' % ndim]) if hp else 0
    avp = av_prior_of(g, table)
    vals, codes = [], []
    for t, b in zip(g['theta%d' % ndim], g['tbox%d' % ndim]):
        v, c = outcome(lambda: orc.logprior(list(t), ns, g['tmin'][b], g['tmax'][b], common.golden_case('A').matrix, avp,
                                            prior=prior, ext=ext, dist_fit=df, rad_prior=rp))
        vals.append(v)
        codes.append(c)
    return np.array(vals), np.array(codes)


@pytest.mark.parametrize('table', [0, 1])
@pytest.mark.parametrize('ndim', [6, 8])
def test_oracle_logprior_every_branch(ndim, table):
    g = prior_golden()
    combos = g['combos%d' % ndim]
    assert len(combos) == 16  # dist_fit x ext x rad_prior x prior list
    bad = []
    for ci in range(len(combos)):
        lp, code = oracle_priors(g, ndim, table, ci)
        want_lp, want_code = g['lp%d' % ndim][table, ci], g['code%d' % ndim][table, ci]
        fin = want_code == OK
        same = (np.array_equal(code, want_code) and np.array_equal(lp == -np.inf, want_lp == -np.inf)
                and rel_err(lp[fin], want_lp[fin]).max(initial=0.0) < 1e-13)
        if not same:
            bad.append((tuple(int(x) for x in combos[ci]), int(np.sum(code != want_code))))
    assert not bad, 'ndim {} table {}: (dist_fit, ext, rad_prior, prior) -> walkers with another outcome: {}'.format(
        ndim, table, bad)


def test_prior_golden_covers_every_outcome_and_gate():
    """The fixture does what it is for: every outcome occurs, each combination rejects some walkers and accepts
    others, and the zero-sigma bins of the variant table change values (mft6.py:1237-1238)."""
    g = prior_golden()
    assert set(np.unique(g['code6'])) == {OK, NEG_INF, VALUEERROR}
    assert set(np.unique(g['code8'])) == {OK, NEG_INF, NONE, VALUEERROR}
    for ndim in (6, 8):
        code = g['code%d' % ndim]
        assert np.all(np.isin(code, (OK, NONE)).any(axis=2)) and np.all((code == NEG_INF).any(axis=2))
        assert np.any(g['av1_sig'] == 0) and not np.any(g['av0_sig'] == 0)
        ext = g['combos%d' % ndim][:, 1] == 1
        both = (code[0] == OK) & (code[1] == OK)
        assert np.any(g['lp%d' % ndim][0][ext][both[ext]] != g['lp%d' % ndim][1][ext][both[ext]])
    # the binary without extinction: the reference gates [A_V, R1], not [R1, ratio] (mft6.py:1219-1227)
    c6 = [tuple(x) for x in g['combos6']]
    on, off = c6.index((1, 1, 0, 0)), c6.index((1, 0, 0, 0))
    assert np.any((g['code6'][0, on] == OK) != (g['code6'][0, off] == OK))


@pytest.mark.parametrize('ndim', [6, 8])
def test_oracle_logposterior_against_the_reference(ndim):
    """Whole posteriors (ndim 6: golden case B; ndim 8: golden case C) with the list prior, per dist_fit / ext /
    rad_prior; the triple with dist_fit and no rad_prior raises TypeError like the reference's np.isfinite(None)."""
    g = prior_golden()
    c = common.golden_case('B' if ndim == 6 else 'C')
    avp = av_prior_of(g, 0)
    prior = list(g['prior%d' % ndim])
    for ci, (df, ext, rp) in enumerate(g['post%d_combos' % ndim]):
        for i, t in enumerate(g['post%d_theta' % ndim]):
            v, code = outcome(lambda: orc.logposterior(
                list(t), c.fr, c.nspec, c.data, c.err, c.r, c.specs, c.ctm, c.ptm, c.tmi, c.tma, c.tmin, c.tmax, c.matrix,
                avp, prior=prior, a=bool(ext), dist_fit=bool(df), rad_prior=bool(rp), bandlib=c.bandlib))
            want, want_code = g['post%d_value' % ndim][ci, i], g['post%d_code' % ndim][ci, i]
            assert code == want_code, (ndim, (df, ext, rp), i)
            if code == OK:
                assert rel_err(v, want) < 1e-13, (ndim, (df, ext, rp), i, v, want)
    if ndim == 8:
        assert np.any(g['post8_code'] == TYPEERROR)
