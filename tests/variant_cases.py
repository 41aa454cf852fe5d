"""One recipe per compiled instance of the hot kernel: what makes the planner of ``mcmc_spec_amd/csrc/msx.hip``
(``pick_block``, ``fused_shape``, ``whole_trips``, ``pf_ok`` / ``pf256_ok``, ``model_in_global``, ``nseg``) take each entry
of ``kVariants``, ``kPairVariants`` and ``kGroupVariants``, and the ``launch_info()['kernel']`` string that entry reports.
``tests/test_variant_cases.py`` holds this table to the three tables of the source (every entry once, nothing else);
``tests/test_gpu_variant_matrix.py`` stages each recipe, asserts that the planner really takes the named instance and pins
its values to the oracle and to the other instances' bits.  Importable without a GPU.

The pixel counts are the smallest that select the instance, from the planner's rules as they stand:

* whole trips (the ``FULL`` entries): no pad pixel and ``npair`` a multiple of the workgroup's trip -- multiples of 1,024 px
  at 256 threads, of 2,048 px at 512 threads and in the linked form's segments; their twins take a ragged count beside it;
* the PF statics (model vector + u + data flux, 8 npix + 32 npair bytes) fit one 512-thread workgroup per CU up to
  5,632 px and two 256-thread ones up to 2,560 px (160 KiB less the kernels' 25,328 / 19,184 bytes of static LDS): 5,633 px
  is the first spectrum a 512-thread workgroup with a CU to itself runs without PF, 3,000 / 3,072 px the ragged / whole-trip
  counts at which two 256-thread workgroups per CU run without it;
* two segments of 8,192 px from 8,193 px on (the linked form; 9,001 ragged, 10,240 whole trips), the model vector in
  global memory from 17,153 px on (GM);
* the pair kernel makes two element trips per lane up to 2,048 px and four up to 4,096 px.

The walker counts are functions of the device's CU count (``Context.device_info()['cus']``) and, for the forms that cut a
batch into sub-batches, of the form's ``walkers_per_sub_batch``."""
from collections import namedtuple

from mcmc_spec_amd import _lib

# kind: 'single' (a context's launch) or 'group' (a target group's).  npix: the pixel count -- of every member, for a
# group.  walkers(cus, rows) -> the walker count -- per member, for a group; rows = the form's walkers_per_sub_batch.
Case = namedtuple('Case', 'id kind nspec npix store broadening path block walkers kernel form')
# The group's device-resident sampler: half_counts(cus) per member; `planned` = the entry plan_group_launch takes for the
# half-counts (Group.launch_info), `runs` = the SMP instance msx_group_sampler_begin launches -- the planned entry's own,
# or the neighbour it substitutes for an entry built without one (without PF, then without SH).
SamplerCase = namedtuple('SamplerCase', 'id nspec npix half_counts planned runs')

MAX_WALKERS_PER_CU = 8     # no case launches more than 8 x CUs walkers
PROBES = 8                 # tests/test_gpu_variant_matrix.py tiles eight probe walkers over every batch


def few(cus, rows):
    """a handful: three copies of the probes, every workgroup with a CU to itself"""
    return min(3 * PROBES, cus)


def half_cu(cus, rows):
    return cus // 2


def over_one_per_cu(cus, rows):
    return cus + 1


def over_two_per_cu(cus, rows):
    return 2 * cus + 1


def straddle(cus, rows):
    """just past one sub-batch of the form, where the device has room for it under MAX_WALKERS_PER_CU"""
    return rows + PROBES if rows + PROBES <= MAX_WALKERS_PER_CU * cus else few(cus, rows)


def pair_of(a, b):
    return lambda cus, rows: (a(cus, rows), b(cus, rows))


FEW_2 = pair_of(lambda cus, rows: 2 * PROBES, lambda cus, rows: 3 * PROBES)             # 40 walkers: <= one per CU
OVER_ONE_2 = pair_of(lambda cus, rows: cus // 2 + 1, lambda cus, rows: cus - cus // 2)   # cus + 1
OVER_TWO_2 = pair_of(lambda cus, rows: cus + 1, lambda cus, rows: cus)                   # 2 cus + 1

W_3CU = 'three workgroups per CU'
W_2CU = 'two per CU, four pixels per lane and trip'
W_2CU_PF = 'two per CU, u / flux staged in LDS during the recipe, four pixels per lane and trip'
W_1CU = 'one workgroup per CU, four pixels per lane and trip'
W_128 = '<= 128 VGPRs: two workgroups fit a CU; rows one star at a time'
W_1CU_PF = 'one workgroup per CU, u / flux staged in LDS during the recipe, four pixels per lane and trip'
W_LINKED = ('one workgroup per walker and 8192-pixel segment; partial sums and histogram counters exchanged inside the '
            'launch; the segment\'s data flux staged in LDS; four pixels per lane and trip')
W_GM = 'model vector in global memory (spectra beyond the LDS), sub-batched'
W_R32 = '; R table stored in float32'
W_FULL = '; whole trips, no clamps'
W_FULL2 = '; whole trips, no clamps in the chi^2 pass'
W_PAIR = ('planner: one thread per walker; two walkers of one grid cell per workgroup, one set of row loads, model values '
          'in registers; two workgroups per CU')


def fused(sig, what):
    return 'logprob_kernel<%s> (%s)' % (sig, what)


def pair(sig):
    return 'pair_plan_kernel + logprob_pair_kernel<512 threads, %s> (%s)' % (sig, W_PAIR)


def group(sig, what):
    return 'logprob_group_kernel<%s> (%s)' % (sig, what)


def _single(id, nspec, npix, store, path, block, walkers, kernel, form=_lib.FORM_FUSED, broadening='staging'):
    return Case(id, 'single', nspec, npix, store, broadening, path, block, walkers, kernel, form)


def _group(id, nspec, npix, block, walkers, kernel):
    return Case(id, 'group', nspec, npix, 'f64', 'staging', _lib.PATH_AUTO, block, walkers, kernel, _lib.FORM_FUSED)


AUTO, FUSED, PAIR, LINKED, INPATH = _lib.PATH_AUTO, _lib.PATH_FUSED, _lib.PATH_PAIR, _lib.PATH_LINKED, _lib.PATH_INPATH
SHARED = _lib.BLOCK_512_SHARED

CASES = (
    # ---- kVariants: the fused binaries and triples ------------------------------------------------------------------
    _single('b256', 2, 1000, 'f64', AUTO, 0, over_two_per_cu, fused('NS=2, 256 threads', W_3CU)),
    _single('b256_sh', 2, 3000, 'f64', AUTO, 256, few, fused('NS=2, 256 threads, SH', W_2CU)),
    _single('b256_sh_pf', 2, 1000, 'f64', AUTO, 0, over_one_per_cu, fused('NS=2, 256 threads, SH, PF', W_2CU_PF)),
    _single('b512', 2, 5633, 'f64', AUTO, 0, half_cu, fused('NS=2, 512 threads', W_1CU)),
    _single('b512_sh', 2, 3000, 'f64', AUTO, 0, over_one_per_cu, fused('NS=2, 512 threads, SH', W_128)),
    _single('b512_pf', 2, 1000, 'f64', AUTO, 0, half_cu, fused('NS=2, 512 threads, PF', W_1CU_PF)),
    _single('t256', 3, 1000, 'f64', AUTO, 0, over_one_per_cu, fused('NS=3, 256 threads', W_3CU)),
    _single('t512', 3, 1000, 'f64', AUTO, SHARED, few, fused('NS=3, 512 threads', W_1CU)),
    _single('t512_pf', 3, 1000, 'f64', AUTO, 0, half_cu, fused('NS=3, 512 threads, PF', W_1CU_PF)),
    # ---- linked, and the model vector in global memory ---------------------------------------------------------------
    _single('b_linked', 2, 9001, 'f64', LINKED, 0, straddle, fused('NS=2, 512 threads, linked', W_LINKED), _lib.FORM_LINKED),
    _single('t_linked', 3, 9001, 'f64', LINKED, 0, straddle, fused('NS=3, 512 threads, linked', W_LINKED), _lib.FORM_LINKED),
    _single('b_gm', 2, 17153, 'f64', FUSED, 0, straddle, fused('NS=2, 512 threads, GM', W_GM)),
    _single('t_gm', 3, 17153, 'f64', FUSED, 0, straddle, fused('NS=3, 512 threads, GM', W_GM)),
    # ---- the float32-stored R table ----------------------------------------------------------------------------------
    _single('r256', 2, 1000, 'f32', AUTO, 0, over_two_per_cu, fused('NS=2, 256 threads, R32', W_3CU + W_R32)),
    _single('r256_sh', 2, 3000, 'f32', AUTO, 256, few, fused('NS=2, 256 threads, SH, R32', W_2CU + W_R32)),
    _single('r256_sh_pf', 2, 1000, 'f32', AUTO, 0, over_one_per_cu, fused('NS=2, 256 threads, SH, PF, R32', W_2CU_PF + W_R32)),
    _single('r512', 2, 5633, 'f32', AUTO, 0, half_cu, fused('NS=2, 512 threads, R32', W_1CU + W_R32)),
    _single('r512_sh', 2, 3000, 'f32', AUTO, 0, over_one_per_cu, fused('NS=2, 512 threads, SH, R32', W_128 + W_R32)),
    _single('r512_pf', 2, 1000, 'f32', AUTO, 0, half_cu, fused('NS=2, 512 threads, PF, R32', W_1CU_PF + W_R32)),
    # ---- whole trips -------------------------------------------------------------------------------------------------
    _single('b256_full', 2, 1024, 'f64', AUTO, 0, over_two_per_cu, fused('NS=2, 256 threads, FULL', W_3CU + W_FULL)),
    _single('b256_sh_full', 2, 3072, 'f64', AUTO, 256, few, fused('NS=2, 256 threads, SH, FULL', W_2CU + W_FULL)),
    _single('b256_sh_pf_full', 2, 1024, 'f64', AUTO, 0, over_one_per_cu, fused('NS=2, 256 threads, SH, PF, FULL', W_2CU_PF + W_FULL)),
    _single('b512_pf_full2', 2, 2048, 'f64', AUTO, 0, half_cu, fused('NS=2, 512 threads, PF, FULL(chi2 pass)', W_1CU_PF + W_FULL2)),
    _single('b512_sh_full2', 2, 2048, 'f64', AUTO, SHARED, few, fused('NS=2, 512 threads, SH, FULL(chi2 pass)', W_128 + W_FULL2)),
    _single('r512_pf_full2', 2, 2048, 'f32', AUTO, 0, half_cu,
            fused('NS=2, 512 threads, PF, R32, FULL(chi2 pass)',
                  'float32-stored grid table R; one workgroup per CU, u / flux staged in LDS' + W_FULL2)),
    _single('b_linked_full2', 2, 10240, 'f64', LINKED, 0, straddle,
            fused('NS=2, 512 threads, linked, FULL(chi2 pass)',
                  'linked: one workgroup per walker and 8192-pixel segment' + W_FULL2), _lib.FORM_LINKED),
    # ---- in-path broadening: the window is the data's own range ------------------------------------------------------
    _single('inpath', 2, 1000, 'f64', INPATH, 0, straddle,
            'inpath_recipe_kernel + inpath_conv_kernel + inpath_resample_kernel + ' +
            fused('NS=2, 512 threads, GIVEN', 'model values given by the in-path broadening kernels; four pixels per lane and trip'),
            _lib.FORM_INPATH, 'in_path'),
    # ---- kPairVariants -----------------------------------------------------------------------------------------------
    _single('pair2', 2, 1000, 'f64', PAIR, 0, few, pair('2 element trips per lane'), _lib.FORM_PAIR),
    _single('pair2_full', 2, 2048, 'f64', PAIR, 0, few, pair('2 element trips per lane, FULL'), _lib.FORM_PAIR),
    _single('pair4', 2, 3000, 'f64', PAIR, 0, few, pair('4 element trips per lane'), _lib.FORM_PAIR),
    _single('pair4_full', 2, 4096, 'f64', PAIR, 0, few, pair('4 element trips per lane, FULL'), _lib.FORM_PAIR),
    # ---- kGroupVariants: two members each; PF and FULL need every member with walkers to qualify ---------------------
    _group('g_b256', 2, (1000, 1024), 0, OVER_TWO_2, group('NS=2, 256 threads', W_3CU)),
    _group('g_b256_sh', 2, (1000, 3000), 256, FEW_2, group('NS=2, 256 threads, SH', W_2CU)),
    _group('g_b256_sh_pf', 2, (1000, 1024), 0, OVER_ONE_2, group('NS=2, 256 threads, SH, PF', W_2CU_PF)),
    _group('g_b512', 2, (1000, 5633), 0, FEW_2, group('NS=2, 512 threads', W_1CU)),
    _group('g_b512_sh', 2, (1000, 3000), 0, OVER_ONE_2, group('NS=2, 512 threads, SH', W_128)),
    _group('g_b512_pf', 2, (1000, 1024), 0, FEW_2, group('NS=2, 512 threads, PF', W_1CU_PF)),
    _group('g_t256', 3, (1000, 1024), 0, OVER_ONE_2, group('NS=3, 256 threads', W_3CU)),
    _group('g_t512', 3, (1000, 1024), SHARED, FEW_2, group('NS=3, 512 threads', W_1CU)),
    _group('g_t512_pf', 3, (1000, 1024), 0, FEW_2, group('NS=3, 512 threads, PF', W_1CU_PF)),
    _group('g_b256_sh_full', 2, (1024, 3072), 256, FEW_2, group('NS=2, 256 threads, SH, FULL', W_2CU + W_FULL)),
    _group('g_b256_sh_pf_full', 2, (1024, 2048), 0, OVER_ONE_2, group('NS=2, 256 threads, SH, PF, FULL', W_2CU_PF + W_FULL)),
    _group('g_b512_pf_full2', 2, (2048, 4096), 0, FEW_2, group('NS=2, 512 threads, PF, FULL(chi2 pass)', W_1CU_PF + W_FULL2)),
    _group('g_b512_sh_full2', 2, (2048, 4096), 0, OVER_ONE_2, group('NS=2, 512 threads, SH, FULL(chi2 pass)', W_128 + W_FULL2)),
)


def half_few(cus):
    return (PROBES, PROBES + 4)


def half_over_one(cus):
    return (cus // 2 + 1, cus - cus // 2)


def half_over_two(cus):
    return (cus + 1, cus)


_PLANNED = {c.id: c.kernel for c in CASES}

# msx_group_sampler_begin plans the members' half-counts with the automatic workgroup size, so only the entries
# pick_block reaches are there: every SMP instance but <NS=2, 256 threads, SH, FULL> (two 256-thread workgroups per CU
# without PF need more than 2,560 px, where pick_block takes 512 threads up to two walkers per CU), and
# <NS=2, 256 threads, SH> only as the substitute of its PF neighbour.
SAMPLER_CASES = (
    SamplerCase('s_b256', 2, (1000, 1024), half_over_two, _PLANNED['g_b256'], 'NS=2, 256 threads'),
    SamplerCase('s_b256_sh_pf_substituted', 2, (1000, 1024), half_over_one, _PLANNED['g_b256_sh_pf'], 'NS=2, 256 threads, SH'),
    SamplerCase('s_b512', 2, (1000, 5633), half_few, _PLANNED['g_b512'], 'NS=2, 512 threads'),
    SamplerCase('s_b512_sh_substituted', 2, (1000, 3000), half_over_one, _PLANNED['g_b512_sh'], 'NS=2, 512 threads'),
    SamplerCase('s_b512_sh_full2_substituted', 2, (2048, 4096), half_over_one, _PLANNED['g_b512_sh_full2'], 'NS=2, 512 threads'),
    SamplerCase('s_b512_pf', 2, (1000, 1024), half_few, _PLANNED['g_b512_pf'], 'NS=2, 512 threads, PF'),
    SamplerCase('s_t256', 3, (1000, 1024), half_over_one, _PLANNED['g_t256'], 'NS=3, 256 threads'),
    # (a 9,001-pixel member: 512 threads whatever the walker count, and its statics do not fit)
    SamplerCase('s_t512', 3, (1000, 9001), half_few, _PLANNED['g_t512'], 'NS=3, 512 threads'),
    SamplerCase('s_t512_pf', 3, (1000, 1024), half_few, _PLANNED['g_t512_pf'], 'NS=3, 512 threads, PF'),
    SamplerCase('s_b256_sh_pf_full', 2, (1024, 2048), half_over_one, _PLANNED['g_b256_sh_pf_full'], 'NS=2, 256 threads, SH, PF, FULL'),
    SamplerCase('s_b512_pf_full2', 2, (2048, 4096), half_few, _PLANNED['g_b512_pf_full2'], 'NS=2, 512 threads, PF, FULL(chi2 pass)'),
)


def by_id(id):
    for c in CASES + SAMPLER_CASES:
        if c.id == id:
            return c
    raise KeyError(id)


def probes(c):
    """The eight probe walkers of a golden case (``common.golden_case('B')`` / ``('C')``): an ordinary one; A_V = 0;
    A_V = 1e-12; the primary's Teff exactly on a grid node; the secondary's halfway between two nodes; the primary on the
    prior box's edge (the comparisons are strict: inside); one the box rejects (R1 < 0.05: -inf as a posterior, a value as
    a likelihood); one outside the isochrone table (rejected by the box as a posterior, ValueError status as a likelihood)."""
    import numpy as np
    ns = c.nspec
    th = np.tile(np.asarray(c.theta[0], dtype=float), (PROBES, 1))
    th[1, ns] = 0.0
    th[2, ns] = 1e-12
    th[3, 0] = 3800.0
    th[4, 1] = 3450.0
    th[5, 0] = c.tmax
    th[6, ns + 1] = 0.04
    th[7, 1] = 2800.0
    return th


FINITE_AS_POSTERIOR = (True,) * 6 + (False,) * 2    # what the oracle must say of the probes (asserted, CPU and GPU)


def synthetic_data(c, npix):
    """npix pixels on the golden grid, over golden case B's wavelength range: (data, err, r), seeded by npix."""
    import numpy as np
    rng = np.random.default_rng(7000 + npix)
    lo, hi = float(np.min(c.data[0])), float(np.max(c.data[0]))
    wl = np.sort(rng.uniform(lo, hi, size=npix))
    data = [wl, 1.0 + 0.1 * rng.normal(size=npix)]
    err = rng.uniform(0.01, 0.2, size=npix)
    return data, err, [wl.min(), wl.max()]
