#!/usr/bin/env python3
"""Launch plans of the hot path: what ``msx_launch_info`` and ``msx_bytes_per_eval`` answer for a matrix of synthetic
problems, walker counts, workgroup sizes and paths.  The plan only depends on the problem's shape (pixels, stars, the R
table's storage), never on its values, so the problems are staged from ``mcmc_spec_amd/synth.py`` with flat data.

    python tests/golden/make_launch_plans.py [out.json [group_out.json]]   # on a GPU (the answers include the kernels' resources)

The group matrix asks ``msx_group_launch_info`` the same of target groups: members that mix pixel counts (whole trips of
a variant or not, LDS-staged statics that fit or not), walker layouts around one and two walkers per CU with empty
members, and every workgroup size.  ``tests/test_gpu_launch_plans.py`` runs both matrices against the library under test
and compares them with the committed ``launch_plans.json`` and ``group_launch_plans.json``.

These files pin WHICH instance a launch takes, not what it computes: the values of every instance are pinned in
``tests/test_gpu_variant_matrix.py`` (one recipe per table entry in ``tests/variant_cases.py``)."""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)

OUT = os.path.join(HERE, 'launch_plans.json')
GROUP_OUT = os.path.join(HERE, 'group_launch_plans.json')
BINARY_PIX = (1194, 2048, 4000, 4096, 16384, 20000)
TRIPLE_PIX = (4096, 16384, 20000)
WALKERS = (16, 128, 256, 384, 512, 1024, 2048, 4096)
INPATH_PIX = 4096
# target groups: (nspec, member pixel counts).  At 256 / 512 threads a binary is whole trips at multiples of 1024 / 2048
# pixels; the PF statics fit two 256-thread workgroups per CU up to ~3,400 pixels and one 512-thread one up to ~6,800.
GROUPS = ((2, (1194, 2048)), (2, (1194, 4096)), (2, (2048, 4096)), (2, (4096, 5120)), (2, (4096, 16384)),
          (2, (5120, 1194, 2048)), (3, (4096, 5120)), (3, (4096, 16384)))
GROUP_TOTALS = (16, 200, 256, 257, 400, 512, 513, 1024, 4096)


def problems():
    """(label, nspec, npix, store, broadening placement) of every staged problem."""
    for npix in BINARY_PIX:
        for store in ('f64', 'f32'):
            yield 'binary', 2, npix, store, 'staging'
    for npix in TRIPLE_PIX:
        yield 'triple', 3, npix, 'f64', 'staging'
    yield 'binary', 2, INPATH_PIX, 'f64', 'in_path'


def _layouts(k):
    """Walker counts per member: every total split evenly, all in the first member, all in the last, one walker in each
    but the last; and no walkers at all."""
    out = []
    for t in GROUP_TOTALS:
        even = [t // k] * k
        even[0] += t - sum(even)
        for c in (even, [t] + [0] * (k - 1), [0] * (k - 1) + [t], [1] * (k - 1) + [t - (k - 1)]):
            if c not in out:
                out.append(c)
    return out + [[0] * k]


def _grid():
    from mcmc_spec_amd import synth
    teffs, loggs = np.arange(3000, 5600, 100), np.array([4.0, 4.5, 5.0, 5.5])
    wl = np.arange(3000, 30000, 0.2)
    return wl, teffs, loggs, synth.make_grid(teffs, loggs, wl)


def _stage(eng, grid, nspec, npix, store, placement):
    from mcmc_spec_amd import bands, synth
    wl, teffs, loggs, flux = grid
    eng.stage_grid(wl, teffs, loggs, flux)
    wl_um = synth.data_wavelengths_um(npix)
    r = [float(wl_um.min()), float(wl_um.max())]
    eng.broaden_grid_window([np.floor(r[0] * 1e4), np.ceil(r[1] * 1e4)], 1700, placement)
    ctm = synth.synthetic_contrast_filters()
    ptm = [[], [], [], []]
    fr = [synth.EXAMPLE_CMAG, synth.EXAMPLE_CERR, ['lp600', 'Kp'], [], [], []]
    tabs, (vw, vf) = synth.synthetic_band_tables(), synth.synthetic_vega()
    ones = np.ones(npix)
    tmi, tma = min(min(w) for w in ctm[0]), max(max(w) for w in ctm[0])
    eng.stage_problem([wl_um, ones], 0.01 * ones, fr, r, ctm, ptm, tmi, tma, synth.make_isochrone_matrix(), nspec=nspec,
                      bands=bands.make_bands(tabs, vw, vf), av_table=synth.make_av_table(), tmin=float(teffs[0]),
                      tmax=float(teffs[-1]), store=store)


def _ask(fn):
    from mcmc_spec_amd import _lib
    try:
        return fn()
    except _lib.MsxError as e:
        return {'error': str(e)}


def collect():
    """Every case of the matrix, in a fixed order: a list of dicts."""
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.engine import Engine
    grid = _grid()
    paths = {'auto': _lib.PATH_AUTO, 'fused': _lib.PATH_FUSED, 'inpath': _lib.PATH_INPATH}
    blocks = (0, 256, 512, _lib.BLOCK_512_SHARED)
    out = []
    for label, nspec, npix, store, placement in problems():
        eng = Engine(0)
        head = {'problem': label, 'nspec': nspec, 'npix': npix, 'store': store, 'broadening': placement}
        try:
            _stage(eng, grid, nspec, npix, store, placement)
        except _lib.MsxError as e:
            out.append(dict(head, stage_error=str(e)))
            eng.ctx.close()
            continue
        for path in (('inpath',) if placement == 'in_path' else ('auto', 'fused')):
            eng.ctx.set_path(paths[path])
            for n in WALKERS:
                for block in ((0,) if path == 'inpath' else blocks):
                    out.append(dict(head, path=path, walkers=n, block=block,
                                    launch_info=_ask(lambda: eng.ctx.launch_info(n, _lib.MODE_LOGPOST, block)),
                                    bytes_per_eval=_ask(lambda: eng.ctx.bytes_per_eval(n))))
        eng.ctx.close()
    return out


def collect_groups():
    """Every case of the group matrix, in a fixed order: a list of dicts."""
    from mcmc_spec_amd import _lib
    from mcmc_spec_amd.engine import Engine
    grid = _grid()
    engines = {}
    for nspec, pix in GROUPS:
        for npix in pix:
            if (nspec, npix) not in engines:
                engines[nspec, npix] = Engine(0)
                _stage(engines[nspec, npix], grid, nspec, npix, 'f64', 'staging')
    out = []
    for nspec, pix in GROUPS:
        grp = _lib.Group([engines[nspec, npix].ctx for npix in pix])
        for counts in _layouts(len(pix)):
            for block in (0, 256, 512, _lib.BLOCK_512_SHARED):
                out.append({'nspec': nspec, 'npix': list(pix), 'counts': counts, 'block': block,
                            'launch_info': _ask(lambda: grp.launch_info(counts, _lib.MODE_LOGPOST, block))})
        grp.close()
    for eng in engines.values():
        eng.ctx.close()
    return out


PER_KERNEL = ('kernel', 'threads', 'vgprs', 'static_lds_bytes')   # a kernel's own attributes, stored once
PER_CASE = ('form_id', 'dynamic_lds_bytes', 'requested_bytes_per_eval', 'workgroups', 'walkers_per_sub_batch')
HEAD = ('problem', 'nspec', 'npix', 'store', 'broadening')


def save(cases, path):
    """One line per problem and path: its cases as rows [walkers, block, form, kernel, dynamic LDS, requested bytes,
    workgroups, walkers per sub-batch, bytes_per_eval]; a kernel's name, threads, VGPRs and static LDS once, in a list of
    their own.  A failed call leaves {"error": message} in place of what it would have returned."""
    kernels, forms, groups = [], {}, {}
    for c in cases:
        key = tuple(c[k] for k in HEAD) + (c.get('path'),)
        g = groups.setdefault(key, dict({k: c[k] for k in HEAD}, **({'path': c['path'], 'rows': []} if 'path' in c else
                                                                     {'stage_error': c.get('stage_error')})))
        if 'path' not in c:
            continue
        li = c['launch_info']
        if 'error' in li:
            info = [li]
        else:
            kern = [li[k] for k in PER_KERNEL]
            if kern not in kernels:
                kernels.append(kern)
            assert forms.setdefault(str(li['form_id']), li['form']) == li['form']
            info = [li['form_id'], kernels.index(kern)] + [li[k] for k in PER_CASE[1:]]
        g['rows'].append([c['walkers'], c['block']] + info + [c['bytes_per_eval']])
    with open(path, 'w') as f:
        f.write('{"forms": ' + json.dumps(forms, sort_keys=True) + ',\n"kernels": [\n' + ',\n'.join(json.dumps(k) for k in kernels) +
                '\n],\n"problems": [\n' + ',\n'.join(json.dumps(g) for g in groups.values()) + '\n]}\n')


def load(path=OUT):
    """The cases of a file save() wrote, in the form collect() returns them."""
    with open(path) as f:
        j = json.load(f)
    out = []
    for g in j['problems']:
        head = {k: g[k] for k in HEAD}
        if 'rows' not in g:
            out.append(dict(head, stage_error=g['stage_error']))
            continue
        for r in g['rows']:
            if isinstance(r[2], dict):
                li = r[2]
            else:
                li = dict(zip(PER_KERNEL, j['kernels'][r[3]]), form=j['forms'][str(r[2])], form_id=r[2],
                          **dict(zip(PER_CASE[1:], r[4:8])))
            out.append(dict(head, path=g['path'], walkers=r[0], block=r[1], launch_info=li, bytes_per_eval=r[-1]))
    return out


GROUP_HEAD = ('nspec', 'npix')


def save_groups(cases, path):
    """One line per group: its cases as rows [counts, block, kernel, dynamic LDS, requested bytes, workgroups, walkers per
    sub-batch] (the form is always the fused one); kernels as in save()."""
    kernels, groups = [], {}
    for c in cases:
        g = groups.setdefault(json.dumps([c[k] for k in GROUP_HEAD]), dict({k: c[k] for k in GROUP_HEAD}, rows=[]))
        li = c['launch_info']
        if 'error' in li:
            info = [li]
        else:
            assert li['form'] == 'fused'
            kern = [li[k] for k in PER_KERNEL]
            if kern not in kernels:
                kernels.append(kern)
            info = [kernels.index(kern)] + [li[k] for k in PER_CASE[1:]]
        g['rows'].append([c['counts'], c['block']] + info)
    with open(path, 'w') as f:
        f.write('{"kernels": [\n' + ',\n'.join(json.dumps(k) for k in kernels) + '\n],\n"groups": [\n' +
                ',\n'.join(json.dumps(g) for g in groups.values()) + '\n]}\n')


def load_groups(path=GROUP_OUT):
    """The cases of a file save_groups() wrote, in the form collect_groups() returns them."""
    from mcmc_spec_amd import _lib
    with open(path) as f:
        j = json.load(f)
    out = []
    for g in j['groups']:
        for r in g['rows']:
            if isinstance(r[2], dict):
                li = r[2]
            else:
                li = dict(zip(PER_KERNEL, j['kernels'][r[2]]), form='fused', form_id=_lib.FORM_FUSED,
                          **dict(zip(PER_CASE[1:], r[3:7])))
            out.append({'nspec': g['nspec'], 'npix': g['npix'], 'counts': r[0], 'block': r[1], 'launch_info': li})
    return out


def main():
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    group_out = sys.argv[2] if len(sys.argv) > 2 else GROUP_OUT
    cases = collect()
    save(cases, out)
    assert load(out) == cases
    print(f'{len(cases)} cases -> {out}')
    groups = collect_groups()
    save_groups(groups, group_out)
    assert load_groups(group_out) == groups
    print(f'{len(groups)} group cases -> {group_out}')


if __name__ == '__main__':
    main()
