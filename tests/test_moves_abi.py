"""CPU: the moves ABI (include/msx.h, msx_*_enqueue_moves*, msx_sampler_draw_moves, msx_move_set): the five functions and
the three constants are declared, exported and mirrored with the right ctypes signatures, and the ctypes mirror of
msx_move_set has the C layout.  No compute calls (no GPU here)."""
import ctypes as C
import inspect
import os
import re
import subprocess
import tempfile

import common  # noqa: F401
from mcmc_spec_amd import _lib, moves

ROOT = common.ROOT
HDR = os.path.join(ROOT, 'include', 'msx.h')

I32P, DP, VP = C.POINTER(C.c_int32), C.POINTER(C.c_double), C.c_void_p
SETP = C.POINTER(moves.MsxMoveSet)
GENERAL = ['const int32_t *sidx', 'const int32_t *cidx', 'const int32_t *kind', 'const int32_t *p1', 'const int32_t *p2',
           'const double *g', 'const double *fac', 'const double *logu']
FUNCTIONS = {
    'msx_sampler_enqueue_moves': (['msx_ctx *ctx', 'int32_t slot', 'int64_t nsteps'] + GENERAL,
                                  [VP, C.c_int32, C.c_int64] + [I32P] * 5 + [DP] * 3),
    'msx_sampler_enqueue_moves_drawn': (['msx_ctx *ctx', 'int32_t slot', 'int64_t nsteps', 'uint64_t seed', 'const msx_move_set *set',
                                         'int64_t first_iter'], [VP, C.c_int32, C.c_int64, C.c_uint64, SETP, C.c_int64]),
    'msx_sampler_draw_moves': (['msx_ctx *ctx', 'uint64_t seed', 'const msx_move_set *set', 'int64_t first_iter', 'int64_t nsteps',
                                'int64_t nw', 'int32_t ndim'] + [p.replace('const ', '') for p in GENERAL],
                               [VP, C.c_uint64, SETP, C.c_int64, C.c_int64, C.c_int64, C.c_int32] + [I32P] * 5 + [DP] * 3),
    'msx_group_sampler_enqueue_moves': (['msx_group *group', 'int32_t slot', 'int64_t nsteps'] + GENERAL,
                                        [VP, C.c_int32, C.c_int64] + [I32P] * 5 + [DP] * 3),
    'msx_group_sampler_enqueue_moves_drawn': (['msx_group *group', 'int32_t slot', 'int64_t nsteps', 'const uint64_t *seeds',
                                               'const msx_move_set *set', 'int64_t first_iter'],
                                              [VP, C.c_int32, C.c_int64, C.POINTER(C.c_uint64), SETP, C.c_int64]),
}


def header():
    return re.sub(r'/\*.*?\*/', '', open(HDR).read(), flags=re.S)


def test_the_five_functions_are_declared_exported_and_mirrored():
    import __graft_entry__ as ge
    ge.build()
    lib = _lib.load()
    txt = header()
    for name, (params, argtypes) in FUNCTIONS.items():
        m = re.search(r'\bint ' + name + r'\s*\(([^)]*)\)\s*;', txt)
        assert m, name
        assert [' '.join(p.split()) for p in m.group(1).split(',')] == params, name
        assert name in _lib.EXPORTED
        fn = getattr(lib, name)
        assert fn.restype is C.c_int and list(fn.argtypes) == argtypes, name


def test_the_wrappers_take_what_the_samplers_pass():
    sig = lambda f: list(inspect.signature(f).parameters)
    general = ['sidx', 'cidx', 'kind', 'p1', 'p2', 'g', 'fac', 'logu']
    assert sig(_lib.Context.sampler_enqueue_moves) == ['self', 'slot'] + general == sig(_lib.Group.sampler_enqueue_moves)
    assert sig(_lib.Context.sampler_enqueue_moves_drawn) == ['self', 'slot', 'nsteps', 'seed', 'moves', 'first_iter']
    assert sig(_lib.Group.sampler_enqueue_moves_drawn) == ['self', 'slot', 'nsteps', 'seeds', 'moves', 'first_iter']
    assert sig(_lib.Context.sampler_draw_moves) == ['self', 'seed', 'moves', 'first_iter', 'nsteps', 'nw', 'ndim']


def test_the_constants_mirror_the_header():
    defs = {m.group(1): int(m.group(2)) for m in re.finditer(r'#define (MSX_M[A-Z_]+) (\d+)', header())}
    assert defs['MSX_MOVE_STRETCH'] == moves.MOVE_STRETCH == _lib.MOVE_STRETCH == moves.StretchMove.kind == 0
    assert defs['MSX_MOVE_DE'] == moves.MOVE_DE == _lib.MOVE_DE == moves.DEMove.kind == 1
    assert defs['MSX_MAX_MOVES'] == moves.MAX_MOVES == _lib.MAX_MOVES == 4
    assert [n for n in defs if n.startswith('MSX_MOVE_')] == ['MSX_MOVE_STRETCH', 'MSX_MOVE_DE']   # every kind has a mirror


def test_move_set_layout_matches_c():
    fields = ['n', 'kind', 'weight', 'a', 'gamma0', 'sigma']
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "msx.h"\nint main(){printf("%zu ' + '%zu ' * len(fields) + \
          '%zu %zu\\n", sizeof(msx_move_set), ' + ', '.join('offsetof(msx_move_set, {})'.format(f) for f in fields) + \
          ', sizeof(((msx_move_set *)0)->kind), sizeof(((msx_move_set *)0)->weight));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, 't.c'), 'w').write(src)
        subprocess.check_call(['gcc', '-I', os.path.join(ROOT, 'include'), '-o', os.path.join(d, 't'), os.path.join(d, 't.c')])
        out = [int(x) for x in subprocess.check_output([os.path.join(d, 't')]).decode().split()]
    S = moves.MsxMoveSet
    assert out == [C.sizeof(S)] + [getattr(S, f).offset for f in fields] + [S.kind.size, S.weight.size]
    assert _lib.MsxMoveSet is S and [f for f, _ in S._fields_] == fields


def test_a_parsed_set_fills_the_struct():
    mset = moves.parse_moves([(moves.StretchMove(2.5), 2.0), (moves.DEMove(), 1.0), (moves.DEMove(sigma=1e-3, gamma0=1.0), 1.0)])
    st = mset.as_struct()
    assert st.n == 3 and list(st.kind)[:3] == [0, 1, 1]
    assert list(st.weight)[:3] == [0.5, 0.25, 0.25] and abs(sum(st.weight) - 1.0) <= 1e-12
    assert st.a[0] == 2.5 and st.gamma0[1] == 0.0 and st.gamma0[2] == 1.0 and st.sigma[1] == 1e-5 and st.sigma[2] == 1e-3
    assert _lib._move_set(st) is st and _lib._move_set(moves.DEMove()).n == 1
