"""GPU: the samplers' posterior analyses are plumbing over the stored-chain view (mcmc_spec_amd/stored.py; DESIGN.md section
27).  Every device sampler family, with the chain resident (autocorr='device') and on the host (autocorr='host'), after a
``sample()`` loop of 12 iterations left after 9 at chunk = 4 -- so that a resident series holds rows past the 9 consumed --
and the selection ``discard=1, thin=2``: four rows, the fewest R-hat takes.

(1) For every analysis and every member selector -- the last rung of the last target among them -- the method's result equals
the module-level function called on ``s._series`` with n = 9 (autocorr='device'), or on ``summary.uploaded(host chain, ctx,
counts)`` (autocorr='host', for the analyses whose host route uploads), with the member indexed by hand: ``np.array_equal`` in
one process.  (2) The two routes of one seeded run agree within the bound the analysis' own test uses.  (3) Rows past the
consumed ones change nothing: the same sampler stopped at 9 rows by ``run_mcmc`` gives the same results.

The engines of test_gpu_loo.py have 6 dimensions and the samplers take no fewer than 2 ndim = 12 walkers
(test_gpu_predictive.NW), so the runs have 12, and [14, 12] for the groups: the smallest unequal pair."""
from contextlib import contextmanager

import numpy as np
import pytest

import common
from mcmc_spec_amd import modes, predictive, products, psis, reweight, summary
from test_gpu_loo import same as same_loo
from test_gpu_modes import EXACT, FLOATS
from test_gpu_predictive import NW, _start
from test_gpu_predictive import same as same_predictive
from test_gpu_products import PRODUCT_COLS, engine
from test_gpu_rank import near as near_rank
from test_gpu_rhat import near as near_moments

pytestmark = pytest.mark.gpu

ITERATIONS, CONSUMED, CHUNK = 12, 9, 4
SEL = dict(discard=1, thin=2)
Q = (0.16, 0.5, 0.84)
COUNTS = [14, 12]
BETAS = [[1.0, 0.5], [1.0, 0.4]]
FAMILIES = ('ensemble', 'group', 'ladder', 'group_ladder')
UPLOADS = ('modes', 'summary', 'products', 'predictive', 'loo', 'reweighted')    # the analyses whose host route uploads the chain


def engines():
    return [engine('B'), engine('A')]


def build(family, autocorr):
    """(the sampler, its initial state)."""
    from mcmc_spec_amd.group import DeviceGroupSampler, TargetGroup
    from mcmc_spec_amd.sampler import DeviceEnsembleSampler
    from mcmc_spec_amd.tempered import DeviceGroupTemperedSampler, DeviceTemperedSampler
    kw = dict(chunk=CHUNK, autocorr=autocorr)
    if family == 'ensemble':
        return DeviceEnsembleSampler(NW, 6, engines()[0], seed=5, **kw), _start(NW)
    if family == 'ladder':
        return DeviceTemperedSampler(NW, 6, engines()[0], betas=BETAS[0], seed=17, **kw), _start(2 * NW, 5).reshape(2, NW, 6)
    if 'group' not in common._cache:
        common._cache['group'] = TargetGroup(engines())
    grp = common._cache['group']
    if family == 'group':
        return DeviceGroupSampler(COUNTS, 6, grp, seeds=[40, 41], **kw), [_start(n, 70 + k) for k, n in enumerate(COUNTS)]
    return (DeviceGroupTemperedSampler(grp, COUNTS, 6, betas=BETAS, seeds=[21, 22], **kw),
            [_start(2 * n, 80 + k).reshape(2, n, 6) for k, n in enumerate(COUNTS)])


def run(family, autocorr, how='left'):
    """The family's sampler after 9 consumed rows: a loop of 12 left after 9, or (how='stopped') ``run_mcmc`` of 9."""
    key = ('stored_chain', family, autocorr, how)
    if key not in common._cache:
        s, p0 = build(family, autocorr)
        if how == 'stopped':
            s.run_mcmc(p0, CONSUMED)
        else:
            for i, _ in enumerate(s.sample(p0, iterations=ITERATIONS)):
                if i == CONSUMED - 1:
                    break
        common._cache[key] = s
    return common._cache[key]


class Subject:
    """One object with the analyses (a sampler, or a group ladder's target), its members and where they lie in the series."""

    def __init__(self, family, s, k=None):
        self.obj = s if k is None else s.target(k)
        self.key = 'k' if family == 'group' else 't'
        self.engines, self.own = engines()[:1], [0]
        self.selectors = [({}, 0)]
        self.host_engines, self.host_counts = self.engines, None
        if family == 'ensemble':
            self.host = lambda: s.get_chain()
        elif family == 'group':
            self.engines, self.own = engines(), [0, 1]
            self.host_engines, self.host_counts = self.engines, COUNTS
            self.host = lambda: np.concatenate([s.get_chain(j) for j in range(2)], axis=1)
        else:
            e, nw = (engines()[0], NW) if k is None else (engines()[k], COUNTS[k])
            self.host_engines, self.host_counts = [e, e], [nw, nw]
            self.host = lambda: self.obj.get_chain(t=None).reshape(CONSUMED, 2 * nw, 6)
            self.engines, self.own = ([e, e], [0, 1]) if k is None else ([g for g in engines() for _ in range(2)], [2 * k, 2 * k + 1])
            self.betas = np.asarray(BETAS[0 if k is None else k])
        if family != 'ensemble':
            self.selectors = [({self.key: None}, None), ({self.key: 0}, 0), ({self.key: 1}, 1)]
        self.ladder = family in ('ladder', 'group_ladder')

    @contextmanager
    def series(self):
        """(series, its members' engines, this subject's members in it): the resident one, or the host chain uploaded."""
        if self.obj._series is not None:
            yield self.obj._series, self.engines, self.own
        else:
            with summary.uploaded(self.host(), self.host_engines[0].ctx, self.host_counts) as (up, n):
                assert n == CONSUMED
                yield up, self.host_engines, list(range(len(self.host_engines)))


def subjects(family, s):
    return [Subject(family, s, k) for k in range(2)] if family == 'group_ladder' else [Subject(family, s)]


def by_hand(out, own, j):
    """Member own[j] (j None: the members own) of a per-member result: a dict of arrays, or a list."""
    idx = own if j is None else own[j]
    if isinstance(out, dict):
        return {name: v[idx] for name, v in out.items() if v is not None}
    return out[idx] if j is not None else [out[i] for i in idx]


def same(got, want, what):
    """Dicts, lists and arrays alike, bit for bit."""
    if isinstance(want, dict):
        assert isinstance(got, dict) and sorted(got) == sorted(want), what
        for name in want:
            same(got[name], want[name], '{}.{}'.format(what, name))
    elif isinstance(want, (list, tuple)):
        assert len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, '{}[{}]'.format(what, i))
    elif want is None or isinstance(want, str):
        assert got == want, what
    else:
        g, w = np.asarray(got), np.asarray(want)
        assert g.shape == w.shape and np.array_equal(g, w, equal_nan=w.dtype.kind == 'f'), what


def moving(chain, counts):
    """(members, ndim): the columns of the host chain (rows, W, ndim) in which every walker of the member has moved."""
    ok = np.ptp(chain, axis=0) > 0.0
    off = np.concatenate([[0], np.cumsum([chain.shape[1]] if counts is None else counts)])
    return np.array([np.all(ok[off[m]:off[m + 1]], axis=0) for m in range(len(off) - 1)])


def fit_arrays(fit):
    return {name: getattr(fit, name) for name in FLOATS + EXACT}


def weights_of(r):
    """What a ``Reweighted`` holds, as arrays; the result is closed."""
    with r:
        return {'members': np.array(r.members), 'stats': dict(r.stats), 'worst': np.asarray(r.worst_status), 'logw': r.logw.read(0, CONSUMED),
                'mean': r.moments(cov=False)['mean']}


def new_engines(sub):
    """(get_reweighted's argument, one engine per own member): each target asked the other target's question."""
    other = [engines()[1], engines()[0]]
    if sub.key == 'k':
        return other, other
    e = other[engines().index(sub.host_engines[0])]
    return e, [e] * len(sub.own)


def analyses(sub, kw):
    """name -> the method's result for the member keywords ``kw``."""
    o = sub.obj
    out = {'tau': o.get_autocorr_time(quiet=True, **SEL, **kw), 'rhat': o.get_rhat(**SEL, **kw), 'moments': o.get_moments(**SEL, **kw),
           'rank_rhat': o.get_rank_rhat(**SEL, **kw), 'mcse': o.get_mcse(q=Q, **SEL, **kw), 'summary': o.get_summary(q=Q, **SEL, **kw),
           'products': o.get_products(PRODUCT_COLS, q=Q, **SEL, **kw), 'predictive': o.get_predictive(q=Q, **SEL, **kw),
           'loo': o.get_loo(**SEL, **kw)}
    for kind in ('bulk', 'tail', 'mean'):
        out['ess_' + kind] = o.get_ess(kind=kind, **SEL, **kw)
    fit = o.get_modes(ncomp=2, cols=[0, 3], **SEL, **kw)
    out['modes'] = fit_arrays(fit)
    fit.close()
    if sub.ladder:
        if kw[sub.key] is not None:
            out['reweighted'] = weights_of(o.get_reweighted(new_engines(sub)[0], **SEL, **kw))
    elif not kw or kw[sub.key] is None:       # (the ensemble's and the group's answer for all members)
        out['reweighted'] = weights_of(o.get_reweighted(new_engines(sub)[0], **SEL))
    return out


def functions(sub, series, engs, own, j):
    """name -> the module-level function on ``series`` with n = 9, member own[j] (None: all of own) indexed by hand."""
    from mcmc_spec_amd.sampler import _device_integrated_time
    n, d, t = CONSUMED, SEL['discard'], SEL['thin']
    one = lambda v: by_hand(v, own, j)
    idx = own if j is None else own[j]
    mom, rr = series.moments(n, d, t, None, True), series.rank_stats(n, d, t, None, (), ('rhat',))
    out = {'tau': _device_integrated_time(series, n, 5.0, d, t)[idx] * t, 'rhat': mom['rhat'][idx],
           'moments': {name: mom[name][idx] for name in ('mean', 'cov', 'count')},
           'rank_rhat': {name: rr[name][idx] for name in ('bulk', 'folded', 'rhat')},
           'summary': one(summary.summary_of(series, n, Q, None, d, t)),
           'products': one(products.summarize_chain(series, n, engs, PRODUCT_COLS, Q, d, t)),
           'predictive': one(predictive.check_series(series, n, engs, Q, d, t)), 'loo': one(psis.loo_series(series, n, engs, d, t, 1.0))}
    st = series.rank_stats(n, d, t, None, Q, ('mcse',))
    out['mcse'] = {'mean': st['mcse_mean'][idx], 'quantiles': st['mcse_quantile'][idx]}
    for kind in ('bulk', 'tail', 'mean'):
        out['ess_' + kind] = series.rank_stats(n, d, t, None, (), (kind,))['ess_' + kind][idx]
    fit = modes.fit_device(series, n, cols=[0, 3], ncomp=2, discard=d, thin=t, ctx=engs[own[0]].ctx)
    out['modes'] = {name: v[[idx] if j is not None else idx] for name, v in fit_arrays(fit).items()}
    new = list(engs)
    for i, e in zip(own, new_engines(sub)[1]):
        new[i] = e
    if sub.ladder:
        if j is not None:
            betas = np.ones(len(engs))
            betas[own] = sub.betas
            out['reweighted'] = weights_of(reweight.of_series(series, n, engs, new, discard=d, thin=t, members=[own[j]], betas=betas))
    elif j is None or sub.key == 't':
        out['reweighted'] = weights_of(reweight.of_series(series, n, engs, new, mode='logposterior', mode_old='logposterior', discard=d, thin=t))
    return out


@pytest.mark.parametrize('autocorr', ['device', 'host'])
@pytest.mark.parametrize('family', FAMILIES)
def test_every_method_is_the_module_function_on_the_series(family, autocorr):
    s = run(family, autocorr)
    for sub in subjects(family, s):
        assert len(sub.host()) == CONSUMED
        if autocorr == 'device':
            assert sub.obj._series.rows > CONSUMED              # (chunks queued past the rows consumed)
        with sub.series() as (series, engs, own):
            for kw, j in sub.selectors:
                got, want = analyses(sub, kw), functions(sub, series, engs, own, j)
                assert sorted(got) == sorted(want)
                for name in got:
                    if autocorr == 'device' or name in UPLOADS:
                        same(got[name], want[name], '{} {} {} {}'.format(family, autocorr, kw, name))


@pytest.mark.parametrize('family', FAMILIES)
def test_the_resident_and_the_uploaded_route_agree(family):
    """One seeded run, the chain resident and on the host.  The analyses that upload make the same device calls on the same
    rows: the same bits (test_gpu_summary, test_gpu_products, test_gpu_predictive, test_gpu_loo, test_gpu_modes and
    test_gpu_reweight compare them so).  The autocorrelation time, the moments and the rank statistics have the host's
    definition on the other side: 1e-9 relative (test_gpu_autocorr's ``rtol`` -- applied to ``tau / thin + 1``, the sum each side
    forms, because four rows leave several tau at zero up to rounding --, test_gpu_rhat.near, test_gpu_rank.near)."""
    dev, host = run(family, 'device'), run(family, 'host')
    for a, b in zip(subjects(family, dev), subjects(family, host)):
        assert np.array_equal(a.host(), b.host())
        for kw, j in a.selectors:
            got, want = analyses(a, kw), analyses(b, kw)
            for name in UPLOADS:
                if name == 'loo':
                    for g, w in zip(*((got[name], want[name]) if isinstance(want[name], list) else ([got[name]], [want[name]]))):
                        same_loo(g, w)
                elif name == 'predictive':
                    for g, w in zip(*((got[name], want[name]) if isinstance(want[name], list) else ([got[name]], [want[name]]))):
                        same_predictive(g, w)
                elif name == 'reweighted':
                    if name in want:
                        want[name]['members'] = got[name]['members']     # (the uploaded series holds the subject's members alone)
                        for part in ('stats', 'worst', 'mean'):
                            same(got[name][part], want[name][part], name + part)
                else:
                    same(got[name], want[name], name)
            # tau = thin (2 sum f - 1): at four rows the sum is 1/2 up to its rounding in several columns, and a relative bound
            # on the few ulp that are left would ask for the same bits; the bound is held to 2 sum f, what each side adds up
            two_sums = [np.asarray(v['tau']) / SEL['thin'] + 1.0 for v in (got, want)]
            assert np.allclose(two_sums[0], two_sums[1], rtol=1e-9, atol=0, equal_nan=True)
            # and tau itself under test_gpu_autocorr's bound over all 9 rows, where it is not degenerate: in the columns in
            # which every walker of the member has moved (a walker that stood still has the autocorrelation 0 / 0, which the
            # rounding of its mean decides on either side)
            moved = moving(a.host(), a.host_counts)
            moved = moved if j is None else moved[j]
            tau9 = [np.asarray(o.obj.get_autocorr_time(quiet=True, **kw)) for o in (a, b)]
            assert tau9[0].shape == tau9[1].shape == moved.shape and np.all(np.abs(tau9[1][moved]) > 1e-3)
            assert np.allclose(tau9[0][moved], tau9[1][moved], rtol=1e-9, atol=0)
            near_moments(got['rhat'], want['rhat'])
            near_moments(got['moments']['mean'], want['moments']['mean'])
            near_moments(got['moments']['cov'], want['moments']['cov'])
            assert np.array_equal(got['moments']['count'], want['moments']['count'])
            for name in ('rank_rhat', 'mcse'):
                for part in want[name]:
                    near_rank(got[name][part], want[name][part], name + '.' + part)
            for kind in ('bulk', 'tail', 'mean'):
                near_rank(got['ess_' + kind], want['ess_' + kind], 'ess_' + kind)


@pytest.mark.parametrize('autocorr', ['device', 'host'])
@pytest.mark.parametrize('family', FAMILIES)
def test_rows_past_the_consumed_ones_change_nothing(family, autocorr):
    left, stopped = run(family, autocorr), run(family, autocorr, 'stopped')
    for a, b in zip(subjects(family, left), subjects(family, stopped)):
        assert np.array_equal(a.host(), b.host()) and len(b.host()) == CONSUMED
        if autocorr == 'device':
            assert a.obj._series.rows > b.obj._series.rows == CONSUMED
        for kw, _ in a.selectors:
            same(analyses(a, kw), analyses(b, kw), '{} {} {}'.format(family, autocorr, kw))
