"""CPU: the device-resident pre-optimiser's ABI surface, the host-side randomness it relies on, and the
one-draw-per-trip restatement (``optimizer.trip_numpy``) against ``fit_spec_batch`` driven by a stub engine.
No GPU here: the kernel itself is checked in tests/test_gpu_opt_device.py."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

import common
from mcmc_spec_amd import _lib, optimizer, synth

ROOT = common.ROOT
ENTRIES = ['msx_opt_run_begin', 'msx_opt_run_enqueue', 'msx_opt_run_collect', 'msx_opt_run_end']


def test_entries_are_declared_exported_and_listed():
    import __graft_entry__ as ge
    ge.build()
    txt = open(os.path.join(ROOT, 'include', 'msx.h')).read()
    txt = re.sub(r'/\*.*?\*/', '', txt, flags=re.S)
    lib = _lib.load()
    for name in ENTRIES:
        assert re.search(r'\b' + name + r'\s*\(', txt), name
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTED, name
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define (MSX_OPT_TRIP_[A-Z]+) (\d+)', open(os.path.join(ROOT, 'include', 'msx.h')).read())}
    assert defs == {'MSX_OPT_TRIP_IDLE': optimizer.TRIP_IDLE, 'MSX_OPT_TRIP_OOB': optimizer.TRIP_OOB,
                    'MSX_OPT_TRIP_REJECTED': optimizer.TRIP_REJECTED, 'MSX_OPT_TRIP_ACCEPTED': optimizer.TRIP_ACCEPTED,
                    'MSX_OPT_TRIP_ERROR': optimizer.TRIP_ERROR}


def test_trip_kernel_instances_do_not_spill():
    """The run adds no instance of the hot kernel (tests/test_abi.py keeps watching those, untouched); its own kernel,
    one thread per chain, keeps the chain's state in registers too: the same -Rpass-analysis reading, ScratchSize 0 and
    not one scratch instruction, for binaries and for triples."""
    src = os.path.join(ROOT, 'mcmc_spec_amd', 'csrc', 'msx.hip')
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, 't.s')
        out = subprocess.run(['/opt/rocm/bin/hipcc', '--offload-arch=gfx950', '-O3', '-std=c++17', '-S', '--cuda-device-only',
                              '-mllvm', '-amdgpu-kernarg-preload-count=8',
                              '-Rpass-analysis=kernel-resource-usage', '-o', asm, src],
                             capture_output=True, text=True)
        assert out.returncode == 0, out.stderr[-2000:]
        text = open(asm).read()
    lines = out.stderr.splitlines()
    seen = 0
    for i, ln in enumerate(lines):
        if 'Function Name' in ln and 'opt_run_trip_kernel' in ln:
            block = '\n'.join(lines[i:i + 14])
            m = re.search(r'ScratchSize \[bytes/lane\]: (\d+)', block)
            assert m and int(m.group(1)) == 0, block
            name = re.search(r'Function Name: (\S+)', ln).group(1)
            body = text[text.index('\n' + name + ':'):]
            body = body[:body.index('.Lfunc_end')]
            assert 'scratch_' not in body, name
            seen += 1
    assert seen == 2  # binaries and triples


@pytest.mark.parametrize('nspec', [2, 3])
@pytest.mark.parametrize('fine', [False, True])
def test_normal_equals_loc_plus_scale_times_standard_normal(nspec, fine):
    """``default_propose``'s four ``rng.normal(gi[n], si[n])`` calls against ``gi + si * standard_normal(ndim)`` on a
    generator in the same state: bit for bit, for the step sizes of both phases -- and a whole chunk drawn at once
    (``standard_normal((k, ndim))``) is the same stream as k calls."""
    ndim = 2 * nspec + 2
    mism = 0
    for seed in range(4):
        a, b, c = (np.random.default_rng(seed) for _ in range(3))
        r = np.random.default_rng(100 + seed)
        chunk = c.standard_normal((500, ndim))
        for k in range(500):
            T = r.uniform(3000, 4200, nspec)
            rad = r.uniform(0.05, 1.0, nspec)
            plx = r.uniform(1 / 3000, 1 / 10)
            gi = [T, r.uniform(0, 1), rad, plx]
            si = optimizer._step_sizes(nspec, list(r.uniform(0.05, 1.0, nspec)), r.uniform(1 / 3000, 1 / 10), fine)
            var = optimizer.default_propose(gi, si, a)
            flat = np.concatenate([np.ravel(v) for v in var])
            z = b.standard_normal(ndim)
            assert np.array_equal(z, chunk[k])
            loc = np.concatenate([np.ravel(v) for v in gi])
            scale = np.array(si[0] + si[1] + si[2] + si[3])
            mism += int(np.sum(flat != loc + scale * z))
    assert mism == 0


# ---- the trip restatement against fit_spec_batch ---------------------------------------------------------------------
TLIM = [3000.0, 4200.0]
DIST_PRIOR = (2.0e-3, 0.1e-3)


def av_table():
    return (np.array([0.0, 100.0, 300.0, 600.0, 1500.0]), np.array([0.05, 0.12, 0.2, 0.31]), np.array([0.02, 0.0, 0.05, 0.1]))


def stand_in(nspec):
    """A deterministic stand-in for the likelihood chi^2 of chain c's proposal `row`: a quadratic bowl whose floor is
    far enough from the start points for both phases to find something to accept."""
    ndim = 2 * nspec + 2
    target = np.array([3900.0, 3500.0, 3300.0][:nspec] + [0.1] + [0.4, 0.6, 0.5][:nspec] + [2.1e-3])
    width = np.array([400.0] * nspec + [0.3] + [0.2] * nspec + [4e-4])

    def f(row, c):
        d = (np.asarray(row, dtype=float)[:ndim] - target) / width
        return float(np.sum(d * d)) * (1.0 + 0.01 * c) + 3.0
    return f


class StubCtx:
    def __init__(self, f):
        self.f = f

    def opt_init(self, starts):
        return np.array([self.f(s, c) for c, s in enumerate(starts)]), np.zeros(len(starts), dtype=np.int32)

    def opt_step(self, batch, owners):
        return np.array([self.f(r, int(c)) for r, c in zip(batch, owners)]), np.zeros(len(batch), dtype=np.int32)


class StubEngine:
    def __init__(self, f):
        self.ctx = StubCtx(f)


def make_starts(nspec, nch, seed):
    """Start points inside the box; the first ones beside its edges: Teff under the upper limit / over the lower one,
    A_V at 0, a radius ratio at 0.05, a parallax far above 1/100 (every out-of-bounds draw then walks the parallax loop
    some 160 times: such a chain runs out of proposals, not of steps)."""
    rng = np.random.default_rng(seed)
    rows = []
    for c in range(nch):
        T = np.sort(rng.uniform(3200, 4000, nspec))[::-1]
        av = rng.uniform(0.05, 0.4)
        rad = [rng.uniform(0.2, 0.9)] + list(rng.uniform(0.2, 0.9, nspec - 1))
        plx = rng.uniform(1.5e-3, 3e-3)
        if c == 0:
            T[0] = 4190.0
        if c == 1:
            T[-1] = 3010.0
        if c == 2:
            av = 0.004
        if c == 3:
            rad[1] = 0.052
        if c == 4:
            plx = 0.05
            av = 0.002
        if c == 5:
            plx = 3.4e-4
        if c == 6 and nspec == 2:
            T = np.array([3500.0, 3510.0])  # T[0] < T[1]: the third loop, once a draw leaves the box
            av = 0.003
        rows.append(list(T) + [av] + rad + [plx])
    return np.array(rows)


class Recorder:
    """A ``propose=`` for fit_spec_batch that is ``default_propose`` and keeps every draw, per chain."""

    def __init__(self, rngs):
        self.ids = {id(r): c for c, r in enumerate(rngs)}
        self.draws = {c: [] for c in range(len(rngs))}

    def __call__(self, gi, si, rng):
        var = optimizer.default_propose(gi, si, rng)
        self.draws[self.ids[id(rng)]].append([np.array(v, dtype=float).copy() for v in var])
        return var


def coverage_of(res, rec, nspec, steps):
    """What fit_spec_batch's own chains and draws show (the conditions of the issue), as a set of names."""
    got = set()
    cap = 50 * steps
    for c, (_, _, ch) in enumerate(res):
        for var in rec.draws[c]:
            if optimizer._in_bounds(var, TLIM):
                if nspec == 3 and (var[2][2] >= var[2][1] or var[2][2] < 0):
                    got.add('third-radius fix')
                continue
            T, av, rad, plx = var
            if np.any(T < min(TLIM)) or np.any(T > max(TLIM)):
                got.add('T loop')
            if av < 0:
                got.add('A_V loop')
            if np.any(rad < 0.05):
                got.add('radius loop')
            if plx > 1 / 100 or plx < 1 / 3000:
                got.add('parallax loop')
        n = 0
        for k, test in enumerate(ch.savetest):
            n += 1
            if test < ch.savechi[k]:
                got.add('fine accept' if n > steps / 2 else 'coarse accept')
                n = steps / 2 + 1 if n > steps / 2 else 0
        assert n == ch.n
        if ch.n >= steps:
            got.add('ends by n')
        elif ch.total_n >= cap:
            got.add('ends by cap')
    return got


def run_both(nspec, steps, nch, seed, rad_prior, dist_fit):
    f = stand_in(nspec)
    starts = make_starts(nspec, nch, seed)
    matrix = synth.make_isochrone_matrix()
    rngs = [np.random.default_rng(1000 * seed + c) for c in range(nch)]
    rec = Recorder(rngs)
    res = optimizer.fit_spec_batch(StubEngine(f), starts, TLIM, DIST_PRIOR, matrix, av_table(), nspec=nspec, steps=steps,
                                   dist_fit=dist_fit, rad_prior=rad_prior, rngs=rngs, propose=rec)
    # the restatement: one draw per trip, every chain until it is idle
    rngs2 = [np.random.default_rng(1000 * seed + c) for c in range(nch)]
    like0 = [f(s, c) for c, s in enumerate(starts)]
    ndim = 2 * nspec + 2
    out = []
    for c in range(nch):
        st = optimizer.TripState(starts[c], optimizer._initial_chi(like0[c], starts[c], DIST_PRIOR, matrix, av_table(), nspec,
                                                                   dist_fit, rad_prior), nspec)
        sp, savechi, savetest = [starts[c].copy()], [st.chi], []
        while True:
            flag, test, _ = optimizer.trip_numpy(st, rngs2[c].standard_normal(ndim), lambda row: f(row, c), TLIM, DIST_PRIOR,
                                                 matrix, av_table(), nspec=nspec, steps=steps, dist_fit=dist_fit,
                                                 rad_prior=rad_prior)
            if flag == optimizer.TRIP_IDLE:
                break
            if flag >= optimizer.TRIP_REJECTED:
                sp.append(st.gi.copy())
                savechi.append(st.chi)
                savetest.append(test)
        out.append((sp, savechi, savetest, st))
    return res, rec, out


def flat(g):
    return np.concatenate([np.ravel(np.asarray(v, dtype=float)) for v in g])


@pytest.mark.parametrize('nspec,steps,rad_prior,dist_fit', [(2, 12, True, True), (2, 7, False, False), (3, 9, True, True)])
def test_trip_restatement_walks_fit_spec_batch_chains(nspec, steps, rad_prior, dist_fit):
    res, rec, out = run_both(nspec, steps, 16, 3, rad_prior, dist_fit)
    for c, ((line, best, ch), (sp, savechi, savetest, st)) in enumerate(zip(res, out)):
        assert len(ch.sp) == len(sp), c
        assert all(np.array_equal(flat(a), b) for a, b in zip(ch.sp, sp)), c
        assert ch.savechi == savechi and ch.savetest == savetest, c
        assert ch.n == st.n and ch.total_n == st.total_n, c
        assert line == optimizer._row_text(optimizer._groups(st.gi, nspec) if len(sp) > 1 else ch.sp[0], nspec) + '\n', c
        assert best == st.chi
    got = coverage_of(res, rec, nspec, steps)
    want = {'T loop', 'A_V loop', 'radius loop', 'parallax loop', 'coarse accept', 'fine accept', 'ends by n', 'ends by cap'}
    if nspec == 3:
        want = {'third-radius fix', 'coarse accept', 'ends by n'}
    assert want <= got, sorted(want - got)


class StubRunCtx(StubCtx):
    """``msx_opt_run_*`` restated with ``trip_numpy``: what fit_spec_device's plumbing (draws per chunk, two slots, the
    chains rebuilt from records and flags, the files) can be checked against without a GPU."""

    def __init__(self, f, matrix, nspec):
        super().__init__(f)
        self.matrix, self.nspec, self.slots = matrix, nspec, {}

    def opt_run_begin(self, gi0, chi0, steps, tlim, dist_fit, rad_prior, dist_prior, av_tab, iso, max_chunk_trips):
        self.st = [optimizer.TripState(g, c, self.nspec) for g, c in zip(gi0, chi0)]
        self.kw = dict(tlim=tlim, dist_prior=dist_prior, matrix=self.matrix, av_table=av_tab, nspec=self.nspec, steps=steps,
                       dist_fit=dist_fit, rad_prior=rad_prior)
        self.cap_trips = max_chunk_trips

    def opt_run_enqueue(self, slot, z):
        assert slot not in self.slots and len(z) <= self.cap_trips
        ndim = 2 * self.nspec + 2
        rec = np.empty((len(z), len(self.st), ndim + 2))
        fl = np.empty((len(z), len(self.st)), dtype=np.int32)
        for t in range(len(z)):
            for c, st in enumerate(self.st):
                fl[t, c], test, _ = optimizer.trip_numpy(st, z[t, c], lambda row: self.f(row, c), **self.kw)
                rec[t, c] = list(st.gi) + [st.chi, test]
        live = sum(1 for st in self.st if not st.done and st.n < self.kw['steps'] and st.total_n < 50 * self.kw['steps'])
        self.slots[slot] = (rec, fl, live, 0)

    def opt_run_collect(self, slot, ntrips):
        return self.slots.pop(slot)

    def opt_run_end(self):
        return (np.array([st.gi for st in self.st]), np.array([st.chi for st in self.st]),
                np.array([float(st.n) for st in self.st]), np.array([st.total_n for st in self.st], dtype=np.int64))


@pytest.mark.parametrize('nspec,steps,chunk', [(2, 12, 16), (3, 9, 1), (2, 7, 5000)])
def test_fit_spec_device_plumbing_rebuilds_fit_spec_batch_results(nspec, steps, chunk, tmp_path):
    f = stand_in(nspec)
    starts = make_starts(nspec, 10, 3)
    matrix = synth.make_isochrone_matrix()
    args = (starts, TLIM, DIST_PRIOR, matrix, av_table())
    kw = dict(nspec=nspec, steps=steps, dist_fit=True, rad_prior=True)
    (tmp_path / 'h').mkdir()
    (tmp_path / 'd').mkdir()
    host = optimizer.fit_spec_batch(StubEngine(f), *args, rngs=[np.random.default_rng(50 + c) for c in range(10)],
                                    dirname=str(tmp_path / 'h'), first_index=3, **kw)
    eng = StubEngine(f)
    eng.ctx = StubRunCtx(f, matrix, nspec)
    dev = optimizer.fit_spec_device(eng, *args, rngs=[np.random.default_rng(50 + c) for c in range(10)],
                                    dirname=str(tmp_path / 'd'), first_index=3, chunk=chunk, **kw)
    for c, ((hl, hb, hc), (dl, db, dc)) in enumerate(zip(host, dev)):
        assert hl == dl and hb == db, c
        assert len(hc.sp) == len(dc.sp) and all(np.array_equal(flat(a), flat(b)) for a, b in zip(hc.sp, dc.sp)), c
        assert hc.savechi == dc.savechi and hc.savetest == dc.savetest and hc.n == dc.n and hc.total_n == dc.total_n, c
        assert dc.trips >= len(dc.savetest)
    names = sorted(os.listdir(tmp_path / 'h'))
    assert names == sorted(os.listdir(tmp_path / 'd')) and 'params3.txt' in names and 'chisq12.txt' in names
    for name in names:
        assert (tmp_path / 'h' / name).read_text() == (tmp_path / 'd' / name).read_text(), name
