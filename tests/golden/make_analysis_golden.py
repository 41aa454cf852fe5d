"""Records tests/golden/analysis_host.npz: every host-route posterior analysis of a seeded run of each host sampler family,
bit for bit (tests/test_analysis_golden.py recomputes it with ``record()`` and compares).  Run it on the commit whose numbers
are to be kept:

    python tests/golden/make_analysis_golden.py

The runs: ``EnsembleSampler`` (8 walkers), ``GroupSampler`` ([8, 6]), ``TemperedSampler`` (8 walkers, 3 rungs) and
``GroupTemperedSampler`` ([8, 6], 2 rungs); 3 dimensions, a Gaussian target, fixed seeds; 41 stored rows, and 3 and 0 stored
rows for what the analyses raise.  A key is ``family:rows:selection:member:analysis[.field]``; an analysis that raises is
recorded as ``[type name, message]`` under ``...!raise``."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NDIM, ROWS = 3, 41
OUT = os.path.join(ROOT, 'tests', 'golden', 'analysis_host.npz')
SELECTIONS = {'all': {}, 'cut': dict(discard=5, thin=2, cols=[2, 0])}


def gauss(x):
    x = np.asarray(x, dtype=float)
    return -0.5 * np.sum((x - 0.25) ** 2, axis=1) / 0.81


def flat_prior(x):
    return np.zeros(len(x))


def start(nw, seed):
    return np.random.default_rng(seed).normal(0.25, 0.9, size=(nw, NDIM))


def families():
    """name -> (run(rows) -> sampler, {member name: (the object to ask, its member keywords)}, has a ladder)."""
    from mcmc_spec_amd.group import GroupSampler
    from mcmc_spec_amd.sampler import EnsembleSampler
    from mcmc_spec_amd.tempered import GroupTemperedSampler, TemperedSampler

    def ensemble(rows):
        s = EnsembleSampler(8, NDIM, gauss, vectorize=True, seed=11)
        s.run_mcmc(start(8, 1), rows)
        return s

    def group(rows):
        s = GroupSampler([8, 6], NDIM, lambda ts: [gauss(t) for t in ts], seeds=[12, 13])
        s.run_mcmc([start(8, 2), start(6, 3)], rows)
        return s

    def ladder(rows):
        s = TemperedSampler(8, NDIM, gauss, flat_prior, ntemps=3, seed=14)
        s.run_mcmc(start(8, 4), rows)
        return s

    def group_ladder(rows):
        s = GroupTemperedSampler([8, 6], NDIM, lambda ts: [gauss(t) for t in ts], lambda ts: [flat_prior(t) for t in ts], ntemps=2,
                                 seeds=[15, 16])
        s.run_mcmc([start(8, 5), start(6, 6)], rows)
        return s

    return {
        'ensemble': (ensemble, lambda s: {'one': (s, {})}, False),
        'group': (group, lambda s: {'every': (s, {}), 'k1': (s, dict(k=1))}, False),
        'tempered': (ladder, lambda s: {'every': (s, dict(t=None)), 't2': (s, dict(t=2))}, True),
        'group_tempered': (group_ladder, lambda s: {'every': (s.target(1), dict(t=None)), 't1': (s.target(1), dict(t=1))}, True),
    }


def analyses(s, who, sel, short):
    """name -> a call of one analysis of ``s`` for the member keywords ``who`` and the selection ``sel``."""
    rows = {k: v for k, v in sel.items() if k != 'cols'}
    out = {
        'tau': lambda: s.get_autocorr_time(quiet=True, **rows, **who),
        'rhat': lambda: s.get_rhat(**sel, **who),
        'moments': lambda: s.get_moments(**sel, **who),
        'rank_rhat': lambda: s.get_rank_rhat(**sel, **who),
        'mcse': lambda: s.get_mcse(**sel, **who),
        'modes': lambda: s.get_modes(**sel, **who),
    }
    for kind in ('bulk', 'tail', 'mean'):
        out['ess_' + kind] = lambda kind=kind: s.get_ess(kind=kind, **sel, **who)
    if short:
        out['tau_loud'] = lambda: s.get_autocorr_time(**rows, **who)
    return out


def ladder_analyses(s, sel):
    rows = {k: v for k, v in sel.items() if k != 'cols'}
    return {'mean_log_like': lambda: s.mean_log_like(**rows),
            'evidence_ti': lambda: s.log_evidence(method='ti', **rows),
            'evidence_ss': lambda: s.log_evidence(method='ss', **rows)}


def put(out, key, call):
    """The result of ``call()`` under ``key``: an array, a dict's or a named tuple's fields, a mode fit's parameters, or the raise."""
    try:
        v = call()
    except Exception as e:   # (whatever it is: its type and message are the record)
        out[key + '!raise'] = np.array([type(e).__name__, str(e)])
        return
    if hasattr(v, 'params'):
        w, mu, cv = v.params()
        v = {'weight': w, 'mean_z': mu, 'cov_z': cv, 'center': v.center, 'scale': v.scale, 'loglik': v.loglik, 'best': v.best}
    elif hasattr(v, '_asdict'):
        v = v._asdict()
    if isinstance(v, dict):
        for name, a in v.items():
            out['{}.{}'.format(key, name)] = np.asarray(a)
    else:
        out[key] = np.asarray(v)


def record():
    out = {}
    for fam, (run, members, has_ladder) in families().items():
        for nrows in (ROWS, 3, 0):
            s = run(nrows)
            short = nrows < ROWS
            for sel_name, sel in SELECTIONS.items():
                if short and sel_name != 'all':
                    continue
                for who_name, (obj, who) in members(s).items():
                    base = '{}:{}:{}:{}:'.format(fam, nrows, sel_name, who_name)
                    for name, call in analyses(obj, who, sel, short).items():
                        put(out, base + name, call)
                if has_ladder:
                    obj = members(s)['every'][0]
                    for name, call in ladder_analyses(obj, sel).items():
                        put(out, '{}:{}:{}:ladder:{}'.format(fam, nrows, sel_name, name), call)
    return out


if __name__ == '__main__':
    rec = record()
    np.savez_compressed(OUT, **rec)
    print('{}: {} arrays, {} raises, {} bytes'.format(OUT, len(rec), sum(k.endswith('!raise') for k in rec), os.path.getsize(OUT)))
