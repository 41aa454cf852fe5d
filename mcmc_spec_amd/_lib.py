"""ctypes binding of ``libmsx.so`` (the C ABI declared in ``include/msx.h``).

There is no CPU fallback: if the HIP library has not been built the import of any compute entry
point fails loudly with the build command.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MSX_LIB overrides the library path (diagnostic builds such as -DMSX_STAMPS; never a CPU fallback)
LIB_PATH = os.environ.get('MSX_LIB') or os.path.join(_HERE, 'libmsx.so')

MSX_OK = 0
MSX_ERR_INVALID, MSX_ERR_HIP, MSX_ERR_STATE, MSX_ERR_RANGE = -1, -2, -3, -4
W_OK, W_REJECT, W_KEYERROR, W_INDEXERROR, W_VALUEERROR, W_HANDOVER = 0, 1, 2, 3, 4, 5
MODE_LOGLIKE, MODE_LOGPOST, MODE_CHISQ, MODE_LOGPRIOR = 0, 1, 2, 3
BLOCK_512_SHARED = 1512  # include/msx.h MSX_BLOCK_512_SHARED: 512 threads, two workgroups per CU
PATH_AUTO, PATH_FUSED, PATH_PAIR, PATH_LINKED, PATH_INPATH = 0, 1, 2, 4, 8  # include/msx.h MSX_PATH_*
BROADEN_STAGING, BROADEN_IN_PATH = 0, 1  # include/msx.h MSX_BROADEN_*
FORM_FUSED, FORM_PAIR, FORM_LINKED, FORM_INPATH = 0, 1, 2, 3  # include/msx.h MSX_FORM_*
STORE_F64, STORE_F32 = 0, 1  # include/msx.h MSX_STORE_*
FORM_NAMES = {0: 'fused', 1: 'pair (planner + two walkers of one grid cell per workgroup)', 2: 'linked (one workgroup per walker and 8192-pixel segment)',
              3: 'in-path broadening (recipe, composite + convolution, resample, then the fused kernel on the given model values)'}
HOOK_LINKED_FAULT, HOOK_PAIR_LEASES = 1, 2  # include/msx.h MSX_HOOK_*
MAX_SPEC, MAX_BANDS, MAX_DIM = 3, 8, 8
MODES_MAX = 4  # MSX_MODES_MAX: the components of a mixture (msx_series_modes)
MAX_GROUP = 64  # include/msx.h MSX_MAX_GROUP: members of a target group
RESAMPLE_TILE = 1024  # include/msx.h MSX_RESAMPLE_TILE: the samples of one tile of msx_series_resample's prefix scan
PSIS_TAIL_MAX, PSIS_MIN_TAIL = 4096, 5  # include/msx.h MSX_PSIS_TAIL_MAX, MSX_PSIS_MIN_TAIL: the longest tail msx_series_psis fits, the shortest
PSIS_LOG_TINY = -708.3964185322641  # include/msx.h MSX_PSIS_LOG_TINY: log of the smallest normal double
POINTWISE_MATRIX_MAX = 1 << 30  # include/msx.h MSX_POINTWISE_MATRIX_MAX: the largest pointwise matrix the calls hand back, bytes
PSIS_OK, PSIS_SHORT_TAIL = 0, 1  # include/msx.h MSX_PSIS_*: a member's status
PB_TRAPZ, PB_SUM, PB_MEAN = 0, 1, 2  # include/msx.h MSX_PB_*: the kinds of a product band
SPEC_MEDIAN_SCALE = 1  # include/msx.h MSX_SPEC_MEDIAN_SCALE
MAX_PCOLS = 64  # include/msx.h MSX_MAX_PCOLS: derived columns of one products_batch call
from .moves import MOVE_STRETCH, MOVE_DE, MAX_MOVES, MsxMoveSet  # noqa: E402  include/msx.h MSX_MOVE_*, MSX_MAX_MOVES, msx_move_set

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int64)
_up = C.POINTER(C.c_uint32)


class MsxProblem(C.Structure):
    """Mirror of ``struct msx_problem`` (include/msx.h) -- keep the field order identical."""
    _fields_ = [
        ('struct_size', C.c_int32), ('nspec', C.c_int32), ('npix', C.c_int64),
        ('pix_lo', _ip), ('pix_t', _dp), ('pix_u', _dp), ('pix_flux', _dp), ('pix_err', _dp),
        ('median_flux', C.c_double), ('fit_minv', C.c_double * 9),
        ('n_contrast', C.c_int32), ('n_phot', C.c_int32),
        ('band_i0', _ip), ('band_len', _ip), ('band_w', _dp),
        ('cmag', _dp), ('cerr', _dp), ('pmag', _dp), ('perr', _dp), ('phot_zero', _dp), ('phot_k', _dp),
        ('win_j0', C.c_int64), ('win_n', C.c_int64),
        ('niso', C.c_int32), ('iso_teff', _dp), ('iso_logg', _dp), ('iso_lum', _dp),
        ('nav', C.c_int32), ('av_edges_pc', _dp), ('av_mu', _dp), ('av_sig', _dp),
        ('tmin', C.c_double), ('tmax', C.c_double),
        ('prior_mean', C.c_double * MAX_DIM), ('prior_sig', C.c_double * MAX_DIM),
        ('use_av', C.c_int32), ('dist_fit', C.c_int32), ('rad_prior', C.c_int32), ('has_prior_list', C.c_int32),
        ('no_spectrum', C.c_int32),
    ]


class MsxProducts(C.Structure):
    """Mirror of ``struct msx_products`` (include/msx.h) -- keep the field order identical."""
    _fields_ = [
        ('struct_size', C.c_int32), ('nbands', C.c_int32),
        ('band_kind', C.POINTER(C.c_int32)), ('band_i0', _ip), ('band_len', _ip), ('band_w', _dp), ('band_zero_mag', _dp),
        ('niso', C.c_int32), ('iso_teff', _dp), ('iso_mass', _dp), ('iso_lum', _dp),
    ]


class MsxError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__('msx error {}: {}'.format(code, msg))
        self.code = code
        self.msg = msg


_lib = None


def load():
    """Load ``libmsx.so`` once.  Raises ImportError with the build recipe if it is missing."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            'mcmc_spec_amd: the HIP library {} is missing. Build it with\n'
            '  python -c "import __graft_entry__ as g; g.build()"   (or: make -C mcmc_spec_amd/csrc)\n'
            'There is no CPU fallback for the log-likelihood path.'.format(LIB_PATH))
    # One HIP runtime per process: PyTorch-ROCm ships its own libamdhip64 (same SONAME as
    # /opt/rocm's).  If torch were imported *after* this library had bound to /opt/rocm's copy the
    # process would hold two runtimes and torch's streams / device pointers would be foreign to
    # ours.  Importing torch first makes the loader resolve our NEEDED entry to the copy torch
    # already mapped.  (torch is plumbing here: device memory, streams, torch.distributed.)
    if os.environ.get('MSX_SKIP_TORCH_IMPORT') is None:
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
    lib = C.CDLL(LIB_PATH)
    vp = C.c_void_p
    sig = {
        'msx_create': (C.c_int, [C.c_int, C.POINTER(vp)]),
        'msx_destroy': (None, [vp]),
        'msx_last_error': (C.c_char_p, [vp]),
        'msx_device_info': (C.c_int, [vp, _ip, C.c_char_p, C.c_int]),
        'msx_stage_grid': (C.c_int, [vp, _dp, C.c_int64, _dp, C.c_int32, _dp, C.c_int32, _dp, C.POINTER(C.c_uint8)]),
        'msx_ccm89_k': (C.c_int, [vp, _dp, C.c_int64, C.c_double, _dp]),
        'msx_resample_linear': (C.c_int, [vp, _dp, _dp, C.c_int64, _dp, C.c_int64, _dp]),
        'msx_broaden': (C.c_int, [vp, _dp, _dp, C.c_int64, C.c_double, C.c_double, _dp]),
        'msx_broaden_grid': (C.c_int, [vp, C.c_int64, C.c_int64, C.c_double, C.c_double]),
        'msx_rot_broaden': (C.c_int, [vp, _dp, _dp, C.c_int64, C.c_double, C.c_double, _dp]),
        'msx_rot_broaden_grid': (C.c_int, [vp, C.c_int64, C.c_int64, C.c_double, C.c_double]),
        'msx_split_components': (C.c_int, [vp, C.c_int32]),
        'msx_stage_grid_components': (C.c_int, [vp, _dp, C.c_int64, _dp, C.c_int32, _dp, C.c_int32, _dp,
                                                C.POINTER(C.c_uint8), C.c_int32]),
        'msx_rot_broaden_grid_component': (C.c_int, [vp, C.c_int32, C.c_int64, C.c_int64, C.c_double, C.c_double]),
        'msx_read_node_component': (C.c_int, [vp, C.c_int32, C.c_int32, C.c_int32, _dp]),
        'msx_read_node': (C.c_int, [vp, C.c_int32, C.c_int32, _dp]),
        'msx_stage_problem': (C.c_int, [vp, C.POINTER(MsxProblem)]),
        'msx_logprob_batch': (C.c_int, [vp, C.c_int32, _dp, C.c_int64, C.c_int32, _dp, C.POINTER(C.c_int32)]),
        'msx_logprob_batch_dev': (C.c_int, [vp, C.c_int32, vp, C.c_int64, C.c_int32, vp, vp, vp, C.c_int32]),
        'msx_probe_launch': (C.c_int, [vp, C.c_int32, vp, C.c_int64, C.c_int32, vp, vp, vp, C.c_int32, _dp]),
        'msx_set_path': (C.c_int, [vp, C.c_int32]),
        'msx_set_grid_storage': (C.c_int, [vp, C.c_int32]),
        'msx_set_broadening': (C.c_int, [vp, C.c_int32]),
        'msx_opt_init': (C.c_int, [vp, _dp, C.c_int64, C.c_int32, _dp, C.POINTER(C.c_int32)]),
        'msx_opt_step': (C.c_int, [vp, _dp, C.POINTER(C.c_int32), C.c_int64, C.c_int32, _dp, C.POINTER(C.c_int32)]),
        'msx_opt_run_begin': (C.c_int, [vp, C.c_int64, C.c_int32, _dp, _dp, C.c_int64, C.c_double, C.c_double, C.c_int32, C.c_int32,
                                        C.c_double, C.c_double, C.c_int32, _dp, C.c_int32, _dp, _dp, C.c_int32, _dp, _dp, C.c_int64]),
        'msx_opt_run_enqueue': (C.c_int, [vp, C.c_int32, C.c_int64, _dp]),
        'msx_opt_run_collect': (C.c_int, [vp, C.c_int32, _dp, C.POINTER(C.c_int32), _ip, C.POINTER(C.c_int32)]),
        'msx_opt_run_end': (C.c_int, [vp, _dp, _dp, _dp, _ip]),
        'msx_sampler_run': (C.c_int, [vp, C.c_int32, C.c_int64, C.c_int32, C.c_int64, _dp, _dp, C.POINTER(C.c_int32),
                                      C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, _dp, _dp, _dp, _dp, _ip,
                                      C.POINTER(C.c_int32)]),
        'msx_sampler_begin': (C.c_int, [vp, C.c_int32, C.c_int64, C.c_int32, C.c_int64, _dp, _dp, _ip]),
        'msx_sampler_shard': (C.c_int, [vp, C.c_int32, C.c_int32]),
        'msx_sampler_enqueue': (C.c_int, [vp, C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                          C.POINTER(C.c_int32), _dp, _dp, _dp]),
        'msx_sampler_collect': (C.c_int, [vp, C.c_int32, _dp, _dp, _ip, C.POINTER(C.c_int32)]),
        'msx_sampler_enqueue_drawn': (C.c_int, [vp, C.c_int32, C.c_int64, C.c_uint64, C.c_double, C.c_int64]),
        'msx_sampler_draw': (C.c_int, [vp, C.c_uint64, C.c_double, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int32),
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, _dp, _dp]),
        'msx_sampler_end': (C.c_int, [vp, _dp, _dp]),
        'msx_sampler_enqueue_moves': (C.c_int, [vp, C.c_int32, C.c_int64] + [C.POINTER(C.c_int32)] * 5 + [_dp, _dp, _dp]),
        'msx_sampler_enqueue_moves_drawn': (C.c_int, [vp, C.c_int32, C.c_int64, C.c_uint64, C.POINTER(MsxMoveSet), C.c_int64]),
        'msx_sampler_draw_moves': (C.c_int, [vp, C.c_uint64, C.POINTER(MsxMoveSet), C.c_int64, C.c_int64, C.c_int64, C.c_int32] +
                                   [C.POINTER(C.c_int32)] * 5 + [_dp, _dp, _dp]),
        'msx_group_sampler_enqueue_moves': (C.c_int, [vp, C.c_int32, C.c_int64] + [C.POINTER(C.c_int32)] * 5 + [_dp, _dp, _dp]),
        'msx_group_sampler_enqueue_moves_drawn': (C.c_int, [vp, C.c_int32, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(MsxMoveSet),
                                                            C.c_int64]),
        'msx_tempered_begin': (C.c_int, [vp, C.c_int32, _dp, C.c_int64, C.c_int32, C.c_int64, _dp, _dp, _dp]),
        'msx_tempered_enqueue': (C.c_int, [vp, C.c_int32, C.c_int64] + [C.POINTER(C.c_int32)] * 5 + [_dp, _dp, _dp, _dp]),
        'msx_tempered_enqueue_drawn': (C.c_int, [vp, C.c_int32, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(MsxMoveSet), C.c_int64]),
        'msx_tempered_draw': (C.c_int, [vp, C.c_int32, C.POINTER(C.c_uint64), C.POINTER(MsxMoveSet), C.c_int64, C.c_int64, C.c_int64,
                                        C.c_int32] + [C.POINTER(C.c_int32)] * 5 + [_dp, _dp, _dp, _dp]),
        'msx_tempered_collect': (C.c_int, [vp, C.c_int32, _dp, _dp, _dp, _ip, _ip, C.POINTER(C.c_int32)]),
        'msx_tempered_end': (C.c_int, [vp, _dp, _dp, _dp]),
        'msx_ladder_adapt': (C.c_int, [vp, C.c_double, C.c_double, C.c_int64]),
        'msx_ladder_betas': (C.c_int, [vp, C.c_int32, _dp]),
        'msx_ladder_current': (C.c_int, [vp, _dp, _ip, _ip]),
        'msx_ladder_step': (C.c_int, [C.c_int32, _dp, _ip, C.c_int64, C.c_int64, C.c_double, C.c_double, _dp, C.POINTER(C.c_int32)]),
        'msx_make_composite': (C.c_int, [vp, _dp, _dp, _dp, C.c_int32, C.c_double, _dp, _dp, _dp,
                                         C.POINTER(C.c_int32)]),
        'msx_comm_unique_id': (C.c_int, [vp, C.POINTER(C.c_uint8)]),
        'msx_comm_init': (C.c_int, [vp, C.POINTER(C.c_uint8), C.c_int32, C.c_int32]),
        'msx_comm_allgather_dev': (C.c_int, [vp, vp, vp, C.c_int64, vp, C.c_int32]),
        'msx_comm_wait_slot': (C.c_int, [vp, C.c_int32, vp]),
        'msx_comm_init_loopback': (C.c_int, [C.POINTER(vp), C.c_int32]),
        'msx_sampler_enqueue_group': (C.c_int, [C.POINTER(vp), C.c_int32, C.c_int32, C.c_int64, C.POINTER(C.c_int32),
                                                C.POINTER(C.c_int32), C.POINTER(C.c_int32), _dp, _dp, _dp]),
        'msx_stream_copy_gbps': (C.c_int, [vp, C.c_int64, C.c_int32, _dp]),
        'msx_bytes_per_eval': (C.c_int, [vp, C.c_int64, _ip]),
        'msx_test_hook': (C.c_int, [vp, C.c_int32, C.c_int32]),
        'msx_launch_info': (C.c_int, [vp, C.c_int32, C.c_int64, C.c_int32, C.c_char_p, C.c_int32, _ip]),
        'msx_last_form': (C.c_int, [vp, C.POINTER(C.c_int32)]),
        'msx_pair_stats': (C.c_int, [vp, _ip]),
        'msx_sampler_overlapped': (C.c_int, [vp, C.POINTER(C.c_int32)]),
        'msx_sampler_policy': (C.c_int, [vp, C.c_int32]),
        'msx_group_create': (C.c_int, [C.POINTER(vp), C.c_int32, C.POINTER(vp)]),
        'msx_group_destroy': (None, [vp]),
        'msx_group_last_error': (C.c_char_p, [vp]),
        'msx_group_logprob_batch': (C.c_int, [vp, C.c_int32, _dp, _ip, C.c_int32, _dp, C.POINTER(C.c_int32)]),
        'msx_group_logprob_batch_dev': (C.c_int, [vp, C.c_int32, vp, _ip, C.c_int32, vp, vp, vp, C.c_int32]),
        'msx_group_launch_info': (C.c_int, [vp, C.c_int32, _ip, C.c_int32, C.c_char_p, C.c_int32, _ip]),
        'msx_group_sampler_begin': (C.c_int, [vp, C.c_int32, _ip, C.c_int32, C.c_int64, _dp, _dp, _ip]),
        'msx_group_sampler_enqueue': (C.c_int, [vp, C.c_int32, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                                C.POINTER(C.c_int32), _dp, _dp, _dp]),
        'msx_group_sampler_enqueue_drawn': (C.c_int, [vp, C.c_int32, C.c_int64, C.POINTER(C.c_uint64), C.c_double, C.c_int64]),
        'msx_group_sampler_collect': (C.c_int, [vp, C.c_int32, _dp, _dp, _ip, C.POINTER(C.c_int32)]),
        'msx_group_sampler_end': (C.c_int, [vp, _dp, _dp]),
        'msx_series_create': (C.c_int, [vp, C.c_int64, C.c_int32, C.c_int32, _ip, C.c_int64, C.POINTER(vp)]),
        'msx_series_destroy': (None, [vp]),
        'msx_series_last_error': (C.c_char_p, [vp]),
        'msx_series_rows': (C.c_int, [vp, _ip]),
        'msx_sampler_attach_series': (C.c_int, [vp, vp, C.c_int64]),
        'msx_group_sampler_attach_series': (C.c_int, [vp, vp, C.c_int64]),
        'msx_series_append': (C.c_int, [vp, _dp, C.c_int64]),
        'msx_series_read': (C.c_int, [vp, C.c_int64, C.c_int64, _dp]),
        'msx_series_acf': (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_int64, C.c_uint32, _dp]),
        'msx_series_order_stats': (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int64, _up, C.c_int32, _ip, C.c_int32, _dp, _ip]),
        'msx_series_hist': (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int64, _up, C.c_int32, _dp, C.c_int32, C.c_int32, _ip]),
        'msx_series_hist2d': (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int64, _up, C.c_int32, _dp, C.c_int32, _dp, C.c_int32,
                                        C.c_int32, _ip]),
        'msx_stage_products': (C.c_int, [vp, C.POINTER(MsxProducts)]),
        'msx_products_batch': (C.c_int, [vp, _dp, C.c_int64, C.c_int32, _up, C.c_int32, _dp, C.POINTER(C.c_int32)]),
        'msx_products_batch_dev': (C.c_int, [vp, vp, C.c_int64, C.c_int32, vp, C.c_int32, vp, vp, vp]),
        'msx_products_spectra': (C.c_int, [vp, _dp, C.c_int64, C.c_int32, C.c_int32, _dp, _dp, C.POINTER(C.c_int32)]),
        'msx_composite_parts': (C.c_int, [vp, _dp, _dp, _dp, C.c_int32, C.c_double, C.c_int64, C.c_int64, _dp, C.POINTER(C.c_int32)]),
        'msx_series_derive': (C.c_int, [vp, C.POINTER(vp), _up, C.c_int32, C.c_int64, C.c_int64, vp, C.POINTER(C.c_int32)]),
        'msx_series_attach_tempered': (C.c_int, [vp, vp, vp, C.c_int64]),
        'msx_series_evidence': (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int64, C.c_int32, _dp, C.c_int32, _dp, _dp]),
        'msx_series_moments': (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int64, _up, C.c_int32, _dp, _dp, _dp, _dp, _dp]),
        'msx_group_tempered_begin': (C.c_int, [vp, C.c_int32, _dp, _ip, C.c_int32, C.c_int64, _dp, _dp, _dp]),
        'msx_group_tempered_enqueue': (C.c_int, [vp, C.c_int32, C.c_int64] + [C.POINTER(C.c_int32)] * 5 + [_dp, _dp, _dp, _dp]),
        'msx_group_tempered_enqueue_drawn': (C.c_int, [vp, C.c_int32, C.c_int64, C.POINTER(C.c_uint64), C.POINTER(MsxMoveSet), C.c_int64]),
        'msx_group_tempered_collect': (C.c_int, [vp, C.c_int32, _dp, _dp, _dp, _ip, _ip, C.POINTER(C.c_int32)]),
        'msx_group_tempered_end': (C.c_int, [vp, _dp, _dp, _dp]),
        'msx_group_tempered_attach_series': (C.c_int, [vp, vp, vp, C.c_int64]),
        'msx_group_ladder_adapt': (C.c_int, [vp, _dp, _dp, _ip]),
        'msx_group_ladder_betas': (C.c_int, [vp, C.c_int32, _dp]),
        'msx_group_ladder_current': (C.c_int, [vp, _dp, _ip, _ip]),
        'msx_predictive_batch': (C.c_int, [vp, _dp, C.c_int64, C.c_int32, _dp, C.c_int32, C.c_int64, _dp, _dp, _dp, _dp,
                                           C.POINTER(C.c_int32), _ip]),
        'msx_series_predictive': (C.c_int, [vp, C.POINTER(vp), C.c_int64, C.c_int64, C.c_int64, _dp, C.c_int32, C.c_int64, _dp, _dp,
                                            _dp, vp, _ip, C.POINTER(C.c_int32)]),
        'msx_series_modes': (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int64, _up, C.c_int32, _dp, _dp, C.c_int32, C.c_int32,
                                       C.POINTER(C.c_int32), _dp, C.c_int32, C.c_double, C.c_double, _dp, _dp, _dp, _dp,
                                       C.POINTER(C.c_int32), C.POINTER(C.c_int32), _ip]),
        'msx_series_mode_labels': (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int64, _up, C.c_int32, _dp, _dp, C.c_int32, _dp, _dp, _dp,
                                             C.POINTER(C.c_uint8), _ip, C.POINTER(vp)]),
        'msx_series_logprob': (C.c_int, [vp, C.POINTER(vp), C.c_int32, C.c_int64, C.c_int64, vp, C.POINTER(C.c_int32)]),
        'msx_series_lincomb': (C.c_int, [C.c_int32, C.POINTER(vp), C.POINTER(C.c_int32), _dp, C.c_int64, C.c_int64, vp]),
        'msx_series_weights': (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int64, vp, _dp]),
        'msx_series_wmoments': (C.c_int, [vp, vp, C.c_int64, C.c_int64, C.c_int64, _up, C.c_int32, _dp, _dp, _dp]),
        'msx_series_resample': (C.c_int, [vp, vp, C.c_int64, C.c_int64, C.c_int64, C.c_uint64, _ip, C.POINTER(vp), _ip]),
        'msx_pointwise_nobs': (C.c_int, [vp, _ip, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
        'msx_predictive_pointwise': (C.c_int, [vp, _dp, C.c_int64, C.c_int32, C.c_double, C.c_int64, _dp, C.POINTER(C.c_int32), _ip, _ip, _dp]),
        'msx_series_pointwise': (C.c_int, [vp, C.POINTER(vp), C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_int64, _dp, _ip, _ip,
                                           C.POINTER(C.c_int32), _dp]),
        'msx_series_psis': (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int64, _ip, vp, vp, _dp, C.POINTER(C.c_int32), _ip, _dp, _ip]),
        'msx_series_split_transform': (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int64, _up, C.c_int32, C.c_int32, _dp, C.c_int64, vp]),
        'msx_split_scratch_bytes': (C.c_int64, [C.c_int64]),
        'msx_series_chain_acov': (C.c_int, [vp, C.c_int64, C.c_int64, C.c_int64, _up, C.c_int32, _dp, _dp, _dp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)  # AttributeError here = header/library skew, fail loudly
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


EXPORTED = ['msx_create', 'msx_destroy', 'msx_last_error', 'msx_device_info', 'msx_stage_grid', 'msx_ccm89_k',
            'msx_resample_linear',
            'msx_broaden', 'msx_broaden_grid', 'msx_rot_broaden', 'msx_rot_broaden_grid', 'msx_split_components',
            'msx_stage_grid_components', 'msx_rot_broaden_grid_component', 'msx_read_node_component', 'msx_read_node', 'msx_stage_problem', 'msx_logprob_batch',
            'msx_logprob_batch_dev', 'msx_probe_launch', 'msx_set_path', 'msx_set_grid_storage', 'msx_set_broadening', 'msx_opt_init', 'msx_opt_step', 'msx_opt_run_begin', 'msx_opt_run_enqueue',
            'msx_opt_run_collect', 'msx_opt_run_end', 'msx_sampler_run', 'msx_sampler_begin',
            'msx_sampler_shard', 'msx_sampler_enqueue', 'msx_sampler_enqueue_drawn', 'msx_sampler_draw', 'msx_sampler_collect', 'msx_sampler_end', 'msx_make_composite', 'msx_comm_unique_id', 'msx_comm_init', 'msx_comm_allgather_dev', 'msx_comm_wait_slot',
            'msx_comm_init_loopback', 'msx_sampler_enqueue_group',
            'msx_stream_copy_gbps', 'msx_bytes_per_eval', 'msx_launch_info', 'msx_last_form', 'msx_test_hook', 'msx_pair_stats', 'msx_sampler_overlapped', 'msx_sampler_policy',
            'msx_group_create', 'msx_group_destroy', 'msx_group_last_error', 'msx_group_logprob_batch',
            'msx_group_logprob_batch_dev', 'msx_group_launch_info', 'msx_group_sampler_begin', 'msx_group_sampler_enqueue',
            'msx_group_sampler_enqueue_drawn', 'msx_group_sampler_collect', 'msx_group_sampler_end',
            'msx_series_create', 'msx_series_destroy', 'msx_series_last_error', 'msx_series_rows', 'msx_sampler_attach_series',
            'msx_group_sampler_attach_series', 'msx_series_append', 'msx_series_read', 'msx_series_acf',
            'msx_series_order_stats', 'msx_series_hist', 'msx_series_hist2d',
            'msx_stage_products', 'msx_products_batch', 'msx_products_batch_dev', 'msx_series_derive',
            'msx_products_spectra', 'msx_composite_parts',
            'msx_sampler_enqueue_moves', 'msx_sampler_enqueue_moves_drawn', 'msx_sampler_draw_moves',
            'msx_group_sampler_enqueue_moves', 'msx_group_sampler_enqueue_moves_drawn',
            'msx_tempered_begin', 'msx_tempered_enqueue', 'msx_tempered_enqueue_drawn', 'msx_tempered_draw', 'msx_tempered_collect',
            'msx_tempered_end', 'msx_series_attach_tempered', 'msx_series_evidence', 'msx_ladder_adapt', 'msx_ladder_betas',
            'msx_ladder_current', 'msx_ladder_step',
            'msx_group_tempered_begin', 'msx_group_tempered_enqueue', 'msx_group_tempered_enqueue_drawn', 'msx_group_tempered_collect',
            'msx_group_tempered_end', 'msx_group_tempered_attach_series', 'msx_group_ladder_adapt', 'msx_group_ladder_betas',
            'msx_group_ladder_current', 'msx_series_moments', 'msx_predictive_batch', 'msx_series_predictive',
            'msx_series_modes', 'msx_series_mode_labels',
            'msx_series_logprob', 'msx_series_lincomb', 'msx_series_weights', 'msx_series_wmoments', 'msx_series_resample',
            'msx_series_psis', 'msx_pointwise_nobs', 'msx_predictive_pointwise', 'msx_series_pointwise',
            'msx_series_split_transform', 'msx_split_scratch_bytes', 'msx_series_chain_acov']


SPLIT_IDENTITY, SPLIT_RANKNORM, SPLIT_FOLD_RANKNORM, SPLIT_INDICATOR, SPLIT_RANK2 = range(5)   # MSX_SPLIT_* (include/msx.h)


def as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def dptr(a):
    return a.ctypes.data_as(_dp)


def iptr(a):
    return a.ctypes.data_as(_ip)


def uptr(a):
    return a.ctypes.data_as(_up)


def col_ratio(a, b):
    """The column code of the derived value x[a] / x[b] (include/msx.h, MSX_COL_RATIO)."""
    a, b = int(a), int(b)
    if not (0 <= a < 256 and 0 <= b < 256):
        raise ValueError('col_ratio: coordinates must lie in 0 .. 255')
    return 0x80000000 | (a << 8) | b


def _pcol(kind, b=0, s=0):
    b, s = int(b), int(s)
    if not (0 <= b < 256 and 0 <= s < 256):
        raise ValueError('derived column: band and star / filter indices must lie in 0 .. 255')
    return (kind << 24) | (b << 8) | s


# the codes of derived columns (include/msx.h, MSX_PCOL_*): b a product band, s a star, f / p a filter / band of the problem
def pcol_bandmag(b, s):
    return _pcol(1, b, s)


def pcol_bandmag_sum(b):
    return _pcol(2, b)


def pcol_dmag(b, s=1):
    return _pcol(3, b, s)


def pcol_pri_corr(b):
    return _pcol(4, b)


def pcol_sec_corr(b):
    return _pcol(5, b)


def pcol_contrast(f):
    return _pcol(6, 0, f)


def pcol_phot(p):
    return _pcol(7, 0, p)


def pcol_logg(s):
    return _pcol(8, 0, s)


def pcol_mass(s):
    return _pcol(9, 0, s)


def pcol_lum(s):
    return _pcol(10, 0, s)


def pcol_decode(code):
    """(kind, band, index) of a derived column's code; kind 0 is a coordinate."""
    code = int(code)
    return code >> 24, (code >> 8) & 0xff, code & 0xff


def _col_codes(cols):
    return np.ascontiguousarray(np.asarray(cols, dtype=np.int64).ravel().astype(np.uint32))


class Context:
    """One ``msx_ctx`` (one device).  Thin, typed wrapper; all numerics happen in the library."""

    def __init__(self, device=0):
        self.lib = load()
        h = C.c_void_p()
        rc = self.lib.msx_create(int(device), C.byref(h))
        self.h = h
        if rc != MSX_OK:
            msg = self.lib.msx_last_error(h).decode() if h else 'allocation failed'
            if h:
                self.lib.msx_destroy(h)
                self.h = None
            raise MsxError(rc, msg)
        self.device = int(device)

    def close(self):
        if getattr(self, 'h', None):
            self.lib.msx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != MSX_OK:
            msg = self.lib.msx_last_error(self.h).decode()
            if rc == MSX_ERR_RANGE:
                raise ValueError(msg)
            raise MsxError(rc, msg)

    # ---- device ---------------------------------------------------------------------------------
    def device_info(self):
        out = np.zeros(3, dtype=np.int64)
        name = C.create_string_buffer(256)
        self.check(self.lib.msx_device_info(self.h, iptr(out), name, 256))
        return {'name': name.value.decode(), 'cus': int(out[0]), 'mem_bytes': int(out[1]), 'clock_khz': int(out[2])}

    def stream_copy_gbps(self, nbytes=1 << 30, iters=10):
        out = C.c_double()
        self.check(self.lib.msx_stream_copy_gbps(self.h, int(nbytes), int(iters), C.byref(out)))
        return out.value

    # ---- grid -----------------------------------------------------------------------------------
    def stage_grid(self, wl, teff_nodes, logg_nodes, flux, present=None):
        wl, teff_nodes, logg_nodes = as_f64(wl), as_f64(teff_nodes), as_f64(logg_nodes)
        flux = as_f64(flux)
        nt, ng, nwl = len(teff_nodes), len(logg_nodes), len(wl)
        if flux.shape != (nt, ng, nwl):
            raise ValueError('flux must be [nt][ng][nwl]')
        pp = None
        if present is not None:
            present = np.ascontiguousarray(present, dtype=np.uint8)
            pp = present.ctypes.data_as(C.POINTER(C.c_uint8))
        self.check(self.lib.msx_stage_grid(self.h, dptr(wl), nwl, dptr(teff_nodes), nt, dptr(logg_nodes), ng,
                                           dptr(flux), pp))
        self.nwl = nwl
        self.ncomp = 1

    def stage_grid_components(self, wl, teff_nodes, logg_nodes, flux, present=None):
        """A component grid from the host: ``flux`` [ncomp][nt][ng][nwl], copy s for star s (``present`` [nt][ng] shared)."""
        wl, teff_nodes, logg_nodes = as_f64(wl), as_f64(teff_nodes), as_f64(logg_nodes)
        flux = as_f64(flux)
        nt, ng, nwl = len(teff_nodes), len(logg_nodes), len(wl)
        if flux.ndim != 4 or flux.shape[1:] != (nt, ng, nwl):
            raise ValueError('flux must be [ncomp][nt][ng][nwl]')
        pp = None
        if present is not None:
            present = np.ascontiguousarray(present, dtype=np.uint8)
            pp = present.ctypes.data_as(C.POINTER(C.c_uint8))
        self.check(self.lib.msx_stage_grid_components(self.h, dptr(wl), nwl, dptr(teff_nodes), nt, dptr(logg_nodes), ng,
                                                      dptr(flux), pp, int(flux.shape[0])))
        self.nwl = nwl
        self.ncomp = int(flux.shape[0])

    def split_components(self, ncomp):
        """Duplicate the staged rows into ``ncomp`` copies, one per star (drops the staged problem)."""
        self.check(self.lib.msx_split_components(self.h, int(ncomp)))
        self.ncomp = int(ncomp)

    def ccm89_k(self, wl, rv=3.1):
        wl = as_f64(np.atleast_1d(wl))
        out = np.empty_like(wl)
        self.check(self.lib.msx_ccm89_k(self.h, dptr(wl), len(wl), float(rv), dptr(out)))
        return out

    def resample_linear(self, x, y, xq):
        x, y, xq = as_f64(x), as_f64(y), as_f64(xq)
        out = np.empty_like(xq)
        self.check(self.lib.msx_resample_linear(self.h, dptr(x), dptr(y), len(x), dptr(xq), len(xq), dptr(out)))
        return out

    def broaden(self, wl, flux, resolution, maxsig=5.0):
        wl, flux = as_f64(wl), as_f64(flux)
        out = np.empty_like(flux)
        self.check(self.lib.msx_broaden(self.h, dptr(wl), dptr(flux), len(wl), float(resolution), float(maxsig),
                                        dptr(out)))
        return out

    def broaden_grid(self, i0, n, resolution, maxsig=5.0):
        self.check(self.lib.msx_broaden_grid(self.h, int(i0), int(n), float(resolution), float(maxsig)))

    def rot_broaden(self, wl, flux, vsini, limb):
        """pyasl.rotBroad(wl, flux, limb, vsini) (edgeHandling 'firstlast'): rotation only; ValueError on a bad vsini / limb."""
        wl, flux = as_f64(wl), as_f64(flux)
        out = np.empty_like(flux)
        self.check(self.lib.msx_rot_broaden(self.h, dptr(wl), dptr(flux), len(wl), float(vsini), float(limb), dptr(out)))
        return out

    def rot_broaden_grid(self, i0, n, vsini, limb):
        self.check(self.lib.msx_rot_broaden_grid(self.h, int(i0), int(n), float(vsini), float(limb)))

    def rot_broaden_grid_component(self, comp, i0, n, vsini, limb):
        self.check(self.lib.msx_rot_broaden_grid_component(self.h, int(comp), int(i0), int(n), float(vsini), float(limb)))

    def read_node_component(self, comp, it, ig):
        out = np.empty(self.nwl)
        self.check(self.lib.msx_read_node_component(self.h, int(comp), int(it), int(ig), dptr(out)))
        return out

    def read_node(self, it, ig):
        out = np.empty(self.nwl)
        self.check(self.lib.msx_read_node(self.h, int(it), int(ig), dptr(out)))
        return out

    # ---- problem + hot path -----------------------------------------------------------------------
    def stage_problem(self, prob: MsxProblem):
        self.check(self.lib.msx_stage_problem(self.h, C.byref(prob)))

    def stage_products(self, prod: MsxProducts):
        self.check(self.lib.msx_stage_products(self.h, C.byref(prod)))

    def products_batch(self, theta, cols):
        """(values (n, ncols), status (n,)): the derived columns ``cols`` (codes) of the samples theta (n, ndim)
        (msx_products_batch); NaN where the status is not W_OK."""
        theta = as_f64(theta)
        cols = _col_codes(cols)
        n, ndim = theta.shape
        out = np.empty((n, cols.size))
        status = np.zeros(n, dtype=np.int32)
        self.check(self.lib.msx_products_batch(self.h, dptr(theta), n, ndim, uptr(cols), cols.size, dptr(out),
                                               status.ctypes.data_as(C.POINTER(C.c_int32))))
        return out, status

    def products_spectra(self, theta, nspec, npix, median_scale=True):
        """(spectra (n, 1 + nspec, npix) in pixel order, scale (n,), status (n,)): msx_products_spectra."""
        theta = as_f64(theta)
        n, ndim = theta.shape
        out = np.empty((n, 1 + int(nspec), int(npix)))
        scale = np.empty(n)
        status = np.zeros(n, dtype=np.int32)
        self.check(self.lib.msx_products_spectra(self.h, dptr(theta), n, ndim, SPEC_MEDIAN_SCALE if median_scale else 0, dptr(out),
                                                 dptr(scale), status.ctypes.data_as(C.POINTER(C.c_int32))))
        return out, scale, status

    def predictive_batch(self, theta, nspec, npix, q=None, scratch_bytes=0):
        """msx_predictive_batch over the samples theta (n, ndim): (band (4, 1 + nspec, npix) = mean, var, min, max, quant
        (len(q), 1 + nspec, npix) or None, resid (3, npix) = the means of data_n, z, z^2, terms (n, 4), status (n,), count),
        reduced over the samples whose status is W_OK.  ``scratch_bytes``: the bound on the temporary device memory (0: the
        library's default)."""
        theta = as_f64(theta)
        n, ndim = theta.shape
        rows = 1 + int(nspec)
        q = None if q is None else as_f64(np.atleast_1d(q))
        band = np.empty((4, rows, int(npix)))
        quant = None if q is None else np.empty((q.size, rows, int(npix)))
        resid = np.empty((3, int(npix)))
        terms = np.empty((n, 4))
        status = np.zeros(n, dtype=np.int32)
        count = np.zeros(1, dtype=np.int64)
        self.check(self.lib.msx_predictive_batch(self.h, dptr(theta), n, ndim, None if q is None else dptr(q), 0 if q is None else q.size,
                                                 int(scratch_bytes), dptr(band), None if quant is None else dptr(quant), dptr(resid),
                                                 dptr(terms), status.ctypes.data_as(C.POINTER(C.c_int32)), iptr(count)))
        return band, quant, resid, terms, status, int(count[0])

    def pointwise_nobs(self):
        """(npix, nc, np): the observations of the staged problem in the pointwise calls' order -- its pixels (0 for a problem
        staged with no_spectrum), contrast filters and photometry bands (msx_pointwise_nobs)."""
        npix, nc, nph = C.c_int64(), C.c_int32(), C.c_int32()
        self.check(self.lib.msx_pointwise_nobs(self.h, C.byref(npix), C.byref(nc), C.byref(nph)))
        return int(npix.value), int(nc.value), int(nph.value)

    def predictive_pointwise(self, theta, reff=1.0, scratch_bytes=0, want_matrix=False):
        """msx_predictive_pointwise over the samples theta (n, ndim): (out (6, n_obs) = lppd, p_waic, elpd_waic, elpd_loo, p_loo,
        khat per observation, status (n,), count, tail_len, the pointwise matrix (n_obs, count) or None)."""
        theta = as_f64(theta)
        n, ndim = theta.shape
        nobs = sum(self.pointwise_nobs())
        out = np.empty((6, nobs))
        status = np.zeros(n, dtype=np.int32)
        count, tail = np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
        ll = np.empty(nobs * n) if want_matrix else None
        self.check(self.lib.msx_predictive_pointwise(self.h, dptr(theta), n, ndim, float(reff), int(scratch_bytes), dptr(out),
                                                     status.ctypes.data_as(C.POINTER(C.c_int32)), iptr(count), iptr(tail),
                                                     None if ll is None else dptr(ll)))
        cnt = int(count[0])
        return out, status, cnt, int(tail[0]), None if ll is None else ll[:nobs * cnt].reshape(nobs, cnt).copy()

    def composite_parts(self, teff, logg, rad, use_distance, plx, j0, n):
        """(parts (nspec, n), status): each star's scaled blend over grid samples [j0, j0 + n) (msx_composite_parts)."""
        teff, logg = as_f64(teff), as_f64(logg)
        r = np.zeros(len(teff))
        r[:len(rad)] = rad
        out = np.empty((len(teff), int(n)))
        status = C.c_int32(0)
        self.check(self.lib.msx_composite_parts(self.h, dptr(teff), dptr(logg), dptr(r), int(bool(use_distance)), float(plx),
                                                int(j0), int(n), dptr(out), C.byref(status)))
        return out, status.value

    def products_batch_dev(self, d_theta_ptr, n, ndim, d_cols_ptr, ncols, d_out_ptr, d_status_ptr, stream_ptr):
        self.check(self.lib.msx_products_batch_dev(self.h, d_theta_ptr, int(n), int(ndim), d_cols_ptr, int(ncols), d_out_ptr,
                                                   d_status_ptr, stream_ptr))

    def logprob_batch(self, theta, mode=MODE_LOGPOST):
        theta = as_f64(theta)
        n, ndim = theta.shape
        logp = np.empty(n)
        status = np.empty(n, dtype=np.int32)
        self.check(self.lib.msx_logprob_batch(self.h, int(mode), dptr(theta), n, ndim, dptr(logp),
                                              status.ctypes.data_as(C.POINTER(C.c_int32))))
        return logp, status

    def logprob_batch_dev(self, d_theta_ptr, n, ndim, d_logp_ptr, d_status_ptr, stream_ptr, mode=MODE_LOGPOST,
                          block_threads=0):
        self.check(self.lib.msx_logprob_batch_dev(self.h, int(mode), C.c_void_p(d_theta_ptr), int(n), int(ndim),
                                                  C.c_void_p(d_logp_ptr), C.c_void_p(d_status_ptr),
                                                  C.c_void_p(stream_ptr), int(block_threads)))

    def set_grid_storage(self, store):
        """'f64' (default) or 'f32': the precision the NEXT stage_problem stores the per-node R table in (msx_set_grid_storage;
        a separately labelled precision -- fused binaries only)."""
        self.check(self.lib.msx_set_grid_storage(self.h, {'f64': STORE_F64, 'f32': STORE_F32}[store]))

    def probe_launch(self, d_theta_ptr, n, ndim, d_logp_ptr, d_status_ptr, stream_ptr, mode=MODE_LOGPOST, block_threads=0):
        """One launch with clock stamps (msx_probe_launch): {'shader_mhz', 'walker_us_median', 'walker_us_max', 'span_us'}."""
        out = np.zeros(4)
        self.check(self.lib.msx_probe_launch(self.h, int(mode), C.c_void_p(d_theta_ptr), int(n), int(ndim), C.c_void_p(d_logp_ptr),
                                             C.c_void_p(d_status_ptr), C.c_void_p(stream_ptr), int(block_threads), dptr(out)))
        return {'shader_mhz': float(out[0]), 'walker_us_median': float(out[1]), 'walker_us_max': float(out[2]), 'span_us': float(out[3])}

    def set_broadening(self, placement):
        """'staging' (default: once per grid node, the reference's live path) or 'in_path' (msx_set_broadening): the next
        broaden_grid also keeps the raw window, and problems staged afterwards have the per-walker form PATH_INPATH."""
        self.check(self.lib.msx_set_broadening(self.h, {'staging': BROADEN_STAGING, 'in_path': BROADEN_IN_PATH}[placement]))

    def set_path(self, path):
        """PATH_AUTO / PATH_FUSED / PATH_PAIR / PATH_LINKED: which form of the hot path launches take (same bits either
        way).  PATH_PAIR (two walkers of one grid cell per workgroup) needs a binary of <= 4096 pixels, PATH_LINKED
        (one workgroup per walker and 8192-pixel segment) a spectrum of 2..8 segments; AUTO picks by batch size."""
        self.check(self.lib.msx_set_path(self.h, int(path)))

    def opt_init(self, theta0):
        theta0 = as_f64(theta0)
        n, ndim = theta0.shape
        chi, status = np.empty(n), np.empty(n, dtype=np.int32)
        self.check(self.lib.msx_opt_init(self.h, dptr(theta0), n, ndim, dptr(chi),
                                         status.ctypes.data_as(C.POINTER(C.c_int32))))
        return chi, status

    def opt_step(self, theta, chain):
        theta = as_f64(theta)
        chain = np.ascontiguousarray(chain, dtype=np.int32)
        n, ndim = theta.shape
        chi, status = np.empty(n), np.empty(n, dtype=np.int32)
        self.check(self.lib.msx_opt_step(self.h, dptr(theta), chain.ctypes.data_as(C.POINTER(C.c_int32)), n, ndim,
                                         dptr(chi), status.ctypes.data_as(C.POINTER(C.c_int32))))
        return chi, status

    def opt_run_begin(self, gi0, chi0, steps, tlim, dist_fit, rad_prior, dist_prior, av_table, iso, max_chunk_trips):
        """Start a device-resident pre-optimiser run (msx_opt_run_begin) over the chains of the last opt_init: gi0
        [nchains][ndim] the start points, chi0 their chi^2 with the prior terms; av_table = (edges, mu, sigma);
        iso = (teff, luminosity) sorted by Teff, or None without rad_prior."""
        gi0, chi0 = as_f64(gi0), as_f64(chi0)
        nch, ndim = gi0.shape
        if chi0.shape != (nch,):
            raise ValueError('opt_run_begin: one chi^2 per start point')
        edges, mu, sig = [as_f64(a) for a in av_table]
        if mu.shape != sig.shape or mu.ndim != 1 or edges.ndim != 1:
            raise ValueError('opt_run_begin: av_table = (edges, mu, sigma), mu and sigma of one length')
        it, il = (None, None) if iso is None else (as_f64(iso[0]), as_f64(iso[1]))
        if it is not None and it.shape != il.shape:
            raise ValueError('opt_run_begin: iso = (teff, luminosity) of one length')
        self.check(self.lib.msx_opt_run_begin(self.h, nch, ndim, dptr(gi0), dptr(chi0), int(steps), float(min(tlim)), float(max(tlim)),
                                              int(bool(dist_fit)), int(bool(rad_prior)), float(dist_prior[0]), float(dist_prior[1]),
                                              edges.size, dptr(edges), mu.size, dptr(mu), dptr(sig),
                                              0 if it is None else it.size, None if it is None else dptr(it),
                                              None if il is None else dptr(il), int(max_chunk_trips)))
        self._opt_shape = (nch, ndim)

    def opt_run_enqueue(self, slot, z):
        """Queue one chunk of trips without waiting for it: z [ntrips][nchains][ndim] standard normals."""
        z = as_f64(z)
        if z.ndim != 3 or z.shape[1:] != self._opt_shape:
            raise ValueError('opt_run_enqueue: z must be [ntrips][nchains][ndim]')
        self.check(self.lib.msx_opt_run_enqueue(self.h, int(slot), z.shape[0], dptr(z)))
        return z.shape[0]

    def opt_run_collect(self, slot, ntrips):
        """Wait for the chunk in `slot`: (records [ntrips][nchains][ndim + 2], flags [ntrips][nchains], live, worst)."""
        nch, ndim = self._opt_shape
        rec = np.empty((int(ntrips), nch, ndim + 2))
        flags = np.empty((int(ntrips), nch), dtype=np.int32)
        live, worst = C.c_int64(), C.c_int32()
        self.check(self.lib.msx_opt_run_collect(self.h, int(slot), dptr(rec), flags.ctypes.data_as(C.POINTER(C.c_int32)),
                                                C.cast(C.byref(live), _ip), C.byref(worst)))
        return rec, flags, live.value, worst.value

    def opt_run_end(self):
        """End the run: (gi [nchains][ndim], chi, n, total_n)."""
        nch, ndim = self._opt_shape
        gi, chi, n, tot = np.empty((nch, ndim)), np.empty(nch), np.empty(nch), np.empty(nch, dtype=np.int64)
        self.check(self.lib.msx_opt_run_end(self.h, dptr(gi), dptr(chi), dptr(n), iptr(tot)))
        return gi, chi, n, tot

    def sampler_run(self, mode, coords, logp, sidx, cidx, partner, zz, zfac, logu):
        """Run len(zz) stretch-move steps on the device.  coords [nw][ndim] and logp [nw] are updated in place;
        returns (chain [nsteps][nw][ndim], logp_chain [nsteps][nw], naccept [nw], worst_status)."""
        i32p = C.POINTER(C.c_int32)
        nsteps = zz.shape[0]
        nw, ndim = coords.shape
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (sidx, cidx, partner)]
        dbl = [as_f64(a) for a in (zz, zfac, logu)]
        chain = np.empty((nsteps, nw, ndim))
        lpc = np.empty((nsteps, nw))
        nacc = np.zeros(nw, dtype=np.int64)
        worst = C.c_int32()
        self.check(self.lib.msx_sampler_run(self.h, int(mode), nw, ndim, nsteps, dptr(coords), dptr(logp),
                                            arrs[0].ctypes.data_as(i32p), arrs[1].ctypes.data_as(i32p),
                                            arrs[2].ctypes.data_as(i32p), dptr(dbl[0]), dptr(dbl[1]), dptr(dbl[2]),
                                            dptr(chain), dptr(lpc), iptr(nacc), C.byref(worst)))
        return chain, lpc, nacc, worst.value

    def sampler_begin(self, mode, coords, logp, max_chunk_steps, naccept=None):
        """Start a pipelined device-resident run (msx_sampler_begin): uploads the ensemble state."""
        coords, logp = as_f64(coords), as_f64(logp)
        nw, ndim = coords.shape
        nacc = None if naccept is None else np.ascontiguousarray(naccept, dtype=np.int64)
        self.check(self.lib.msx_sampler_begin(self.h, int(mode), nw, ndim, int(max_chunk_steps), dptr(coords), dptr(logp),
                                              None if nacc is None else iptr(nacc)))
        self._smp_shape = (nw, ndim)

    def sampler_overlapped(self):
        """1 if the run in flight overlaps its half-steps (msx_sampler_overlapped), 0 if not, -1 before its first chunk."""
        out = C.c_int32()
        self.check(self.lib.msx_sampler_overlapped(self.h, C.byref(out)))
        return out.value

    def sampler_policy(self, overlap=-1):
        """-1: overlap consecutive half-steps when the library's rule allows (default); 0: never (a device shared with other work)."""
        self.check(self.lib.msx_sampler_policy(self.h, int(overlap)))

    def sampler_shard(self, rank, world):
        """Shard the run begun by sampler_begin over `world` ranks (msx_sampler_shard); world > 1 needs comm_init."""
        self.check(self.lib.msx_sampler_shard(self.h, int(rank), int(world)))

    def sampler_enqueue(self, slot, sidx, cidx, partner, zz, zfac, logu):
        """Queue one chunk (arrays of shape (nsteps, 2, nw/2)) without waiting for it."""
        return _sampler_enqueue(self, self.lib.msx_sampler_enqueue, 'nwalkers/2', slot, (sidx, cidx, partner, zz, zfac, logu))

    def sampler_enqueue_drawn(self, slot, nsteps, seed, a, first_iter):
        """Queue one chunk whose randomness the device draws itself (msx_sampler_enqueue_drawn): the chunk's first step is
        the ABSOLUTE iteration ``first_iter`` of the seed's stream, which the caller carries across chunks and runs."""
        self.check(self.lib.msx_sampler_enqueue_drawn(self.h, int(slot), int(nsteps), int(seed) & 0xffffffffffffffff, float(a),
                                                      int(first_iter)))
        return int(nsteps)

    def sampler_draw(self, seed, a, first_iter, nsteps, nw, ndim):
        """The device generator's stream for iterations [first_iter, first_iter + nsteps): (sidx, cidx, partner, zz, zfac,
        logu), each (nsteps, 2, nw/2) -- what EnsembleSampler._draw_steps returns."""
        i32p = C.POINTER(C.c_int32)
        shp = (int(nsteps), 2, int(nw) // 2)
        ints = [np.empty(shp, dtype=np.int32) for _ in range(3)]
        dbl = [np.empty(shp) for _ in range(3)]
        self.check(self.lib.msx_sampler_draw(self.h, int(seed) & 0xffffffffffffffff, float(a), int(first_iter), int(nsteps), int(nw), int(ndim),
                                             ints[0].ctypes.data_as(i32p), ints[1].ctypes.data_as(i32p), ints[2].ctypes.data_as(i32p),
                                             dptr(dbl[0]), dptr(dbl[1]), dptr(dbl[2])))
        return tuple(ints) + tuple(dbl)

    def sampler_enqueue_moves(self, slot, sidx, cidx, kind, p1, p2, g, fac, logu):
        """Queue one chunk in the general layout (msx_sampler_enqueue_moves): kind (nsteps,), the others (nsteps, 2, nw/2)."""
        return _sampler_enqueue_moves(self, self.lib.msx_sampler_enqueue_moves, 1, slot, (sidx, cidx, kind, p1, p2, g, fac, logu))

    def sampler_enqueue_moves_drawn(self, slot, nsteps, seed, moves, first_iter):
        """Queue one chunk of a set of moves whose randomness the device draws (msx_sampler_enqueue_moves_drawn): ``moves``
        as the samplers' ``moves=``; the chunk's first step is the ABSOLUTE iteration ``first_iter`` of the seed's stream."""
        st = _move_set(moves)
        self.check(self.lib.msx_sampler_enqueue_moves_drawn(self.h, int(slot), int(nsteps), int(seed) & 0xffffffffffffffff, C.byref(st),
                                                            int(first_iter)))
        return int(nsteps)

    def sampler_draw_moves(self, seed, moves, first_iter, nsteps, nw, ndim):
        """The device generator's stream for a set of moves, iterations [first_iter, first_iter + nsteps): the general
        layout (sidx, cidx, kind, p1, p2, g, fac, logu) -- what EnsembleSampler(moves=...)._draw_steps returns."""
        i32p = C.POINTER(C.c_int32)
        shp = (int(nsteps), 2, int(nw) // 2)
        sidx, cidx, p1, p2 = (np.empty(shp, dtype=np.int32) for _ in range(4))
        kind = np.empty(int(nsteps), dtype=np.int32)
        g, fac, logu = (np.empty(shp) for _ in range(3))
        st = _move_set(moves)
        self.check(self.lib.msx_sampler_draw_moves(self.h, int(seed) & 0xffffffffffffffff, C.byref(st), int(first_iter), int(nsteps), int(nw),
                                                   int(ndim), *[a.ctypes.data_as(i32p) for a in (sidx, cidx, kind, p1, p2)], dptr(g),
                                                   dptr(fac), dptr(logu)))
        return sidx, cidx, kind, p1, p2, g, fac, logu

    def sampler_collect(self, slot, nsteps):
        """Wait for the chunk in `slot`: (chain [nsteps][nw][ndim], logp [nsteps][nw], naccept [nw], worst)."""
        chain, lpc, nacc = _collect_out(self._smp_shape, nsteps)
        worst = C.c_int32()
        self.check(self.lib.msx_sampler_collect(self.h, int(slot), dptr(chain), dptr(lpc), iptr(nacc), C.byref(worst)))
        return chain, lpc, nacc, worst.value

    def sampler_end(self, want_state=False):
        return _sampler_end(self, self.lib.msx_sampler_end, want_state)

    def sampler_attach_series(self, series, at_row):
        """Append every chunk of the run begun by sampler_begin to ``series`` from row ``at_row`` on (msx_sampler_attach_series)."""
        self.check(self.lib.msx_sampler_attach_series(self.h, series.h, int(at_row)))

    # ---- parallel tempering (msx_tempered_*; mcmc_spec_amd.tempered) -------------------------------------------------
    def tempered_begin(self, betas, coords, ll, lpr, max_chunk_steps):
        """Start a tempered run (msx_tempered_begin): coords (T, nw, ndim), ll, lpr (T, nw).  Plain launches:
        ``sampler_policy(0)`` must have been set."""
        betas, coords, ll, lpr = as_f64(betas), as_f64(coords), as_f64(ll), as_f64(lpr)
        T, nw, ndim = coords.shape
        if betas.shape != (T,) or ll.shape != (T, nw) or lpr.shape != (T, nw):
            raise ValueError('tempered_begin: betas (T,), coords (T, nw, ndim), ll and lpr (T, nw)')
        self.check(self.lib.msx_tempered_begin(self.h, T, dptr(betas), nw, ndim, int(max_chunk_steps), dptr(coords), dptr(ll), dptr(lpr)))
        self._tmp_shape = (T, nw, ndim)

    def tempered_enqueue(self, slot, sidx, cidx, kind, p1, p2, g, fac, logu, swap_logu):
        """Queue one host-drawn chunk (msx_tempered_enqueue): kind (nsteps, T), swap_logu (nsteps, T - 1, nw), the others
        (nsteps, T, 2, nw / 2)."""
        i32p = C.POINTER(C.c_int32)
        T, nw, _ = self._tmp_shape
        ints = [np.ascontiguousarray(a, dtype=np.int32) for a in (sidx, cidx, kind, p1, p2)]
        dbl = [as_f64(a) for a in (g, fac, logu, swap_logu)]
        nsteps = dbl[0].shape[0]
        for a in [ints[0], ints[1], ints[3], ints[4]] + dbl[:3]:
            if a.shape != (nsteps, T, 2, nw // 2):
                raise ValueError('tempered_enqueue: arrays must have shape (nsteps, T, 2, walkers / 2)')
        if ints[2].shape != (nsteps, T) or dbl[3].shape != (nsteps, T - 1, nw):
            raise ValueError('tempered_enqueue: kind (nsteps, T), swap_logu (nsteps, T - 1, walkers)')
        self.check(self.lib.msx_tempered_enqueue(self.h, int(slot), nsteps, *[a.ctypes.data_as(i32p) for a in ints], *[dptr(a) for a in dbl]))
        return nsteps

    def tempered_enqueue_drawn(self, slot, nsteps, seeds, moves, first_iter):
        """Queue one chunk whose randomness the device draws (msx_tempered_enqueue_drawn): rung t from ``seeds[t]``, the swap
        draws from ``seeds[0]``; the chunk's first step is the ABSOLUTE iteration ``first_iter``."""
        seeds = np.array([int(s) & 0xffffffffffffffff for s in seeds], dtype=np.uint64)
        if seeds.shape != (self._tmp_shape[0],):
            raise ValueError('tempered_enqueue_drawn: one seed per rung')
        st = _move_set(moves)
        self.check(self.lib.msx_tempered_enqueue_drawn(self.h, int(slot), int(nsteps), seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                       C.byref(st), int(first_iter)))
        return int(nsteps)

    def tempered_draw(self, seeds, moves, first_iter, nsteps, nw, ndim):
        """The device's stream for a ladder of ``len(seeds)`` rungs, iterations [first_iter, first_iter + nsteps): ``(members,
        swap_logu)`` -- members[t] the general layout of rung t (what ``sampler_draw_moves(seeds[t], ...)`` returns) and
        swap_logu (nsteps, T - 1, nw): what ``TemperedSampler(draws=...)`` takes."""
        i32p = C.POINTER(C.c_int32)
        seeds = np.array([int(s) & 0xffffffffffffffff for s in seeds], dtype=np.uint64)
        T, m = len(seeds), int(nsteps)
        shp = (m, T, 2, int(nw) // 2)
        sidx, cidx, p1, p2 = (np.empty(shp, dtype=np.int32) for _ in range(4))
        kind = np.empty((m, T), dtype=np.int32)
        g, fac, logu = (np.empty(shp) for _ in range(3))
        swap = np.empty((m, T - 1, int(nw)))
        st = _move_set(moves)
        self.check(self.lib.msx_tempered_draw(self.h, T, seeds.ctypes.data_as(C.POINTER(C.c_uint64)), C.byref(st), int(first_iter), m, int(nw),
                                              int(ndim), *[a.ctypes.data_as(i32p) for a in (sidx, cidx, kind, p1, p2)], dptr(g), dptr(fac),
                                              dptr(logu), dptr(swap)))
        members = [tuple(np.ascontiguousarray(a[:, t]) for a in (sidx, cidx, kind, p1, p2, g, fac, logu)) for t in range(T)]
        return members, swap

    def tempered_collect(self, slot, nsteps):
        """Wait for the chunk in `slot`: (chain [nsteps][T][nw][ndim], ll, lpr [nsteps][T][nw], naccept [T][nw], nswap [T-1],
        worst [T]); the counts run since begin."""
        T, nw, ndim = self._tmp_shape
        chain, llc, lprc = np.empty((nsteps, T, nw, ndim)), np.empty((nsteps, T, nw)), np.empty((nsteps, T, nw))
        nacc, nswap, worst = np.zeros((T, nw), dtype=np.int64), np.zeros(T - 1, dtype=np.int64), np.zeros(T, dtype=np.int32)
        self.check(self.lib.msx_tempered_collect(self.h, int(slot), dptr(chain), dptr(llc), dptr(lprc), iptr(nacc), iptr(nswap),
                                                 worst.ctypes.data_as(C.POINTER(C.c_int32))))
        return chain, llc, lprc, nacc, nswap, worst

    def tempered_end(self, want_state=False):
        """End the run (msx_tempered_end); its final (coords, ll, lpr) if want_state."""
        if not want_state:
            self.check(self.lib.msx_tempered_end(self.h, None, None, None))
            return None
        T, nw, ndim = self._tmp_shape
        coords, ll, lpr = np.empty((T, nw, ndim)), np.empty((T, nw)), np.empty((T, nw))
        self.check(self.lib.msx_tempered_end(self.h, dptr(coords), dptr(ll), dptr(lpr)))
        return coords, ll, lpr

    def tempered_adapt(self, lag, time, k0):
        """Make the run begun by tempered_begin adaptive from ``k0`` adaptive iterations done (msx_ladder_adapt; DESIGN.md
        section 19): once, before the first enqueue."""
        self.check(self.lib.msx_ladder_adapt(self.h, float(lag), float(time), int(k0)))

    def tempered_betas(self, slot, nsteps):
        """(nsteps, T): the ladders the iterations of the chunk last collected from ``slot`` ran with (msx_ladder_betas)."""
        out = np.empty((int(nsteps), self._tmp_shape[0]))
        self.check(self.lib.msx_ladder_betas(self.h, int(slot), dptr(out)))
        return out

    def tempered_ladder(self):
        """(betas (T,), k, skipped): the run's ladder behind everything queued (msx_ladder_current; it waits for the GPU)."""
        betas, k, skipped = np.empty(self._tmp_shape[0]), np.zeros(1, dtype=np.int64), np.zeros(1, dtype=np.int64)
        self.check(self.lib.msx_ladder_current(self.h, dptr(betas), iptr(k), iptr(skipped)))
        return betas, int(k[0]), int(skipped[0])

    def tempered_attach_series(self, chain, dens, at_row):
        """Append every chunk of the run begun by tempered_begin to the series ``chain`` (T members of nw walkers, ndim) and
        ``dens`` (the same members, ndim 2: ll, lpr) from row ``at_row`` on (msx_series_attach_tempered); either may be None."""
        self.check(self.lib.msx_series_attach_tempered(self.h, None if chain is None else chain.h, None if dens is None else dens.h,
                                                       int(at_row)))

    def make_composite(self, teff, logg, rad, use_distance, plx, win_n, nc, nph):
        teff, logg, rad = as_f64(teff), as_f64(logg), as_f64(rad)
        spec = np.empty(win_n)
        con = np.empty(max(nc, 1))
        ph = np.empty(max(nph, 1))
        st = C.c_int32()
        self.check(self.lib.msx_make_composite(self.h, dptr(teff), dptr(logg), dptr(rad), int(bool(use_distance)),
                                               float(plx), dptr(spec), dptr(con), dptr(ph), C.byref(st)))
        return spec, con[:nc], ph[:nph], st.value

    # ---- RCCL all-gather ------------------------------------------------------------------------------
    def comm_unique_id(self):
        buf = (C.c_uint8 * 128)()
        self.check(self.lib.msx_comm_unique_id(self.h, buf))
        return bytes(buf)

    def comm_init(self, id128, rank, world):
        buf = (C.c_uint8 * 128).from_buffer_copy(bytes(id128))
        self.check(self.lib.msx_comm_init(self.h, buf, int(rank), int(world)))

    # ---- loopback group: the ranks of a sharded run as contexts of one process (include/msx.h) ---------
    @staticmethod
    def comm_init_loopback(contexts):
        """``contexts[r]`` becomes rank r of a loopback group of ``len(contexts)`` ranks (all on one device)."""
        arr = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
        contexts[0].check(contexts[0].lib.msx_comm_init_loopback(arr, len(contexts)))

    @staticmethod
    def sampler_enqueue_group(contexts, slot, sidx, cidx, partner, zz, zfac, logu):
        """One chunk on every rank of a loopback group, in lock-step (arrays as for sampler_enqueue)."""
        i32p = C.POINTER(C.c_int32)
        arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in (sidx, cidx, partner)]
        dbl = [as_f64(a) for a in (zz, zfac, logu)]
        nsteps = dbl[0].shape[0]
        harr = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
        contexts[0].check(contexts[0].lib.msx_sampler_enqueue_group(
            harr, len(contexts), int(slot), nsteps, arrs[0].ctypes.data_as(i32p), arrs[1].ctypes.data_as(i32p),
            arrs[2].ctypes.data_as(i32p), dptr(dbl[0]), dptr(dbl[1]), dptr(dbl[2])))
        return nsteps

    def bytes_per_eval(self, n=256):
        """Bytes the variant an automatic launch of ``n`` walkers takes requests from the memory system, per walker."""
        out = C.c_int64()
        self.check(self.lib.msx_bytes_per_eval(self.h, int(n), C.byref(out)))
        return out.value

    def launch_info(self, n, mode=MODE_LOGPOST, block_threads=0):
        """What an automatic launch of ``n`` walkers would take, from the library's own launcher (msx_launch_info)."""
        out = np.zeros(8, dtype=np.int64)
        name = C.create_string_buffer(512)
        self.check(self.lib.msx_launch_info(self.h, int(mode), int(n), int(block_threads), name, 512, iptr(out)))
        return {'kernel': name.value.decode(), 'form': FORM_NAMES[int(out[0])], 'form_id': int(out[0]), 'threads': int(out[1]),
                'vgprs': int(out[2]), 'static_lds_bytes': int(out[3]), 'dynamic_lds_bytes': int(out[4]),
                'requested_bytes_per_eval': int(out[5]), 'workgroups': int(out[6]), 'walkers_per_sub_batch': int(out[7])}

    def last_form(self):
        """The form (FORM_*) the last launch queued on this context took."""
        out = C.c_int32()
        self.check(self.lib.msx_last_form(self.h, C.byref(out)))
        return out.value

    def pair_stats(self):
        """(pairs, singles) of the pair form's last launch (its planner's counts)."""
        out = np.zeros(2, dtype=np.int64)
        self.check(self.lib.msx_pair_stats(self.h, iptr(out)))
        return int(out[0]), int(out[1])

    def test_hook(self, what, value):
        self.check(self.lib.msx_test_hook(self.h, int(what), int(value)))


class Group:
    """One ``msx_group`` (include/msx.h, target groups): the walkers of several staged contexts on one device, each
    against its own problem, in one launch.  The contexts must stay open while the group is used; closing one, or
    staging its problem again, makes the group refuse every launch (MsxError, MSX_ERR_STATE)."""

    def __init__(self, contexts):
        self.lib = load()
        contexts = list(contexts)
        arr = (C.c_void_p * len(contexts))(*[c.h for c in contexts])
        h = C.c_void_p()
        rc = self.lib.msx_group_create(arr, len(contexts), C.byref(h))
        self.h = h
        self.k = len(contexts)
        if rc != MSX_OK:
            msg = self.lib.msx_group_last_error(h).decode() if h else 'allocation failed'
            if h:
                self.lib.msx_group_destroy(h)
                self.h = None
            raise ValueError(msg) if rc == MSX_ERR_RANGE else MsxError(rc, msg)

    def close(self):
        if getattr(self, 'h', None):
            self.lib.msx_group_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != MSX_OK:
            msg = self.lib.msx_group_last_error(self.h).decode()
            if rc == MSX_ERR_RANGE:
                raise ValueError(msg)
            raise MsxError(rc, msg)

    def _counts(self, counts):
        counts = np.ascontiguousarray(counts, dtype=np.int64)
        if counts.shape != (self.k,):
            raise ValueError('one walker count per member ({} given, {} members)'.format(counts.size, self.k))
        return counts

    def logprob_batch(self, theta, counts, mode=MODE_LOGPOST):
        """theta [sum(counts)][ndim]: member 0's walkers first, then member 1's, ... -> (logp, status)."""
        theta = as_f64(theta)
        counts = self._counts(counts)
        n, ndim = theta.shape
        logp = np.empty(n)
        status = np.empty(n, dtype=np.int32)
        self.check(self.lib.msx_group_logprob_batch(self.h, int(mode), dptr(theta), iptr(counts), ndim, dptr(logp),
                                                    status.ctypes.data_as(C.POINTER(C.c_int32))))
        return logp, status

    def logprob_batch_dev(self, d_theta_ptr, counts, ndim, d_logp_ptr, d_status_ptr, stream_ptr, mode=MODE_LOGPOST,
                          block_threads=0):
        counts = self._counts(counts)
        self.check(self.lib.msx_group_logprob_batch_dev(self.h, int(mode), C.c_void_p(d_theta_ptr), iptr(counts), int(ndim),
                                                        C.c_void_p(d_logp_ptr), C.c_void_p(d_status_ptr),
                                                        C.c_void_p(stream_ptr), int(block_threads)))

    def launch_info(self, counts, mode=MODE_LOGPOST, block_threads=0):
        """What a launch of ``counts`` walkers per member would take (msx_group_launch_info), in Context.launch_info's keys."""
        counts = self._counts(counts)
        out = np.zeros(8, dtype=np.int64)
        name = C.create_string_buffer(512)
        self.check(self.lib.msx_group_launch_info(self.h, int(mode), iptr(counts), int(block_threads), name, 512, iptr(out)))
        return {'kernel': name.value.decode(), 'form': FORM_NAMES[int(out[0])], 'form_id': int(out[0]), 'threads': int(out[1]),
                'vgprs': int(out[2]), 'static_lds_bytes': int(out[3]), 'dynamic_lds_bytes': int(out[4]),
                'requested_bytes_per_eval': int(out[5]), 'workgroups': int(out[6]), 'walkers_per_sub_batch': int(out[7])}

    # ---- the group's device-resident sampler (msx_group_sampler_*) ----
    def sampler_begin(self, mode, coords, logp, counts, max_chunk_steps, naccept=None):
        """Start a run over the group (msx_group_sampler_begin): coords [sum(counts)][ndim] and logp [sum(counts)], member
        0's walkers first."""
        coords, logp = as_f64(coords), as_f64(logp)
        counts = self._counts(counts)
        n, ndim = coords.shape
        if logp.shape != (n,) or int(counts.sum()) != n:
            raise ValueError('sampler_begin: coords, logp and counts disagree')
        nacc = None if naccept is None else np.ascontiguousarray(naccept, dtype=np.int64)
        self.check(self.lib.msx_group_sampler_begin(self.h, int(mode), iptr(counts), ndim, int(max_chunk_steps), dptr(coords),
                                                    dptr(logp), None if nacc is None else iptr(nacc)))
        self._smp_shape = (n, ndim)

    def sampler_enqueue(self, slot, sidx, cidx, partner, zz, zfac, logu):
        """Queue one chunk: arrays (nsteps, 2, sum(counts)/2), the members' active halves side by side, indices member-local."""
        return _sampler_enqueue(self, self.lib.msx_group_sampler_enqueue, 'sum(counts)/2', slot, (sidx, cidx, partner, zz, zfac, logu))

    def sampler_enqueue_drawn(self, slot, nsteps, seeds, a, first_iter):
        """Queue one chunk whose randomness the device draws itself (msx_group_sampler_enqueue_drawn): member m from
        ``seeds[m]``, the chunk's first step the ABSOLUTE iteration ``first_iter`` of every member's stream."""
        seeds = np.ascontiguousarray([int(s) & 0xffffffffffffffff for s in seeds], dtype=np.uint64)
        if seeds.shape != (self.k,):
            raise ValueError('one seed per member ({} given, {} members)'.format(seeds.size, self.k))
        self.check(self.lib.msx_group_sampler_enqueue_drawn(self.h, int(slot), int(nsteps), seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                            float(a), int(first_iter)))
        return int(nsteps)

    def sampler_enqueue_moves(self, slot, sidx, cidx, kind, p1, p2, g, fac, logu):
        """Queue one chunk in the general layout (msx_group_sampler_enqueue_moves): kind (nsteps, k), the others (nsteps, 2,
        sum(counts)/2), the members' active halves side by side, indices member-local."""
        return _sampler_enqueue_moves(self, self.lib.msx_group_sampler_enqueue_moves, self.k, slot, (sidx, cidx, kind, p1, p2, g, fac, logu))

    def sampler_enqueue_moves_drawn(self, slot, nsteps, seeds, moves, first_iter):
        """Queue one chunk of a set of moves whose randomness the device draws (msx_group_sampler_enqueue_moves_drawn): member m
        from ``seeds[m]``, the chunk's first step the ABSOLUTE iteration ``first_iter`` of every member's stream."""
        seeds = np.ascontiguousarray([int(s) & 0xffffffffffffffff for s in seeds], dtype=np.uint64)
        if seeds.shape != (self.k,):
            raise ValueError('one seed per member ({} given, {} members)'.format(seeds.size, self.k))
        st = _move_set(moves)
        self.check(self.lib.msx_group_sampler_enqueue_moves_drawn(self.h, int(slot), int(nsteps), seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                                  C.byref(st), int(first_iter)))
        return int(nsteps)

    def sampler_collect(self, slot, nsteps):
        """Wait for the chunk in `slot`: (chain [nsteps][n][ndim], logp [nsteps][n], naccept [n], worst [k])."""
        chain, lpc, nacc = _collect_out(self._smp_shape, nsteps)
        worst = np.zeros(self.k, dtype=np.int32)
        self.check(self.lib.msx_group_sampler_collect(self.h, int(slot), dptr(chain), dptr(lpc), iptr(nacc),
                                                      worst.ctypes.data_as(C.POINTER(C.c_int32))))
        return chain, lpc, nacc, worst

    def sampler_end(self, want_state=False):
        return _sampler_end(self, self.lib.msx_group_sampler_end, want_state)

    def sampler_attach_series(self, series, at_row):
        """Append every chunk of the group's run to ``series`` from row ``at_row`` on (msx_group_sampler_attach_series)."""
        self.check(self.lib.msx_group_sampler_attach_series(self.h, series.h, int(at_row)))

    # ---- every target's ladder in one run (msx_group_tempered_*; mcmc_spec_amd.tempered.DeviceGroupTemperedSampler) ----
    # The layout is target-major, rung-minor: member m = k T + t owns counts[k] walkers; walkers W = sum T counts[k], proposals
    # per half-step H = W / 2, swap draws per iteration SW = sum (T - 1) counts[k].
    def tempered_begin(self, betas, counts, coords, ll, lpr, max_chunk_steps):
        """Start a tempered run over the group (msx_group_tempered_begin): betas (K, T), counts (K,) walkers per rung, coords
        (W, ndim), ll and lpr (W,)."""
        betas, coords, ll, lpr = as_f64(betas), as_f64(coords), as_f64(ll), as_f64(lpr)
        counts = self._counts(counts)
        if betas.ndim != 2 or betas.shape[0] != self.k or coords.ndim != 2:
            raise ValueError('tempered_begin: betas (K, T), coords (W, ndim)')
        T = betas.shape[1]
        W, ndim = coords.shape
        if W != T * int(counts.sum()) or ll.shape != (W,) or lpr.shape != (W,):
            raise ValueError('tempered_begin: coords (W, ndim), ll and lpr (W,) with W = T * sum(counts)')
        self.check(self.lib.msx_group_tempered_begin(self.h, T, dptr(betas), iptr(counts), ndim, int(max_chunk_steps), dptr(coords), dptr(ll),
                                                     dptr(lpr)))
        self._tmp_shape = (T, [int(n) for n in counts], ndim)

    def tempered_enqueue(self, slot, sidx, cidx, kind, p1, p2, g, fac, logu, swap_logu):
        """Queue one host-drawn chunk (msx_group_tempered_enqueue): kind (nsteps, K T), swap_logu (nsteps, SW), the others
        (nsteps, 2, H), the members' halves side by side, indices member-local."""
        i32p = C.POINTER(C.c_int32)
        T, counts, _ = self._tmp_shape
        ints = [np.ascontiguousarray(a, dtype=np.int32) for a in (sidx, cidx, kind, p1, p2)]
        dbl = [as_f64(a) for a in (g, fac, logu, swap_logu)]
        nsteps = dbl[0].shape[0]
        for a in [ints[0], ints[1], ints[3], ints[4]] + dbl[:3]:
            if a.shape != (nsteps, 2, T * sum(counts) // 2):
                raise ValueError('tempered_enqueue: arrays must have shape (nsteps, 2, T * sum(counts) / 2)')
        if ints[2].shape != (nsteps, self.k * T) or dbl[3].shape != (nsteps, (T - 1) * sum(counts)):
            raise ValueError('tempered_enqueue: kind (nsteps, K T), swap_logu (nsteps, (T - 1) * sum(counts))')
        self.check(self.lib.msx_group_tempered_enqueue(self.h, int(slot), nsteps, *[a.ctypes.data_as(i32p) for a in ints], *[dptr(a) for a in dbl]))
        return nsteps

    def tempered_enqueue_drawn(self, slot, nsteps, seeds, moves, first_iter):
        """Queue one chunk whose randomness the device draws (msx_group_tempered_enqueue_drawn): seeds (K, T), member (k, t) from
        ``seeds[k][t]``, target k's swap draws from ``seeds[k][0]``; ``first_iter`` the chunk's first ABSOLUTE iteration."""
        seeds = np.array([[int(s) & 0xffffffffffffffff for s in row] for row in seeds], dtype=np.uint64)
        if seeds.shape != (self.k, self._tmp_shape[0]):
            raise ValueError('tempered_enqueue_drawn: one seed per target and rung')
        st = _move_set(moves)
        self.check(self.lib.msx_group_tempered_enqueue_drawn(self.h, int(slot), int(nsteps), seeds.ctypes.data_as(C.POINTER(C.c_uint64)),
                                                             C.byref(st), int(first_iter)))
        return int(nsteps)

    def tempered_collect(self, slot, nsteps):
        """Wait for the chunk in `slot`: (chain [nsteps][W][ndim], ll, lpr [nsteps][W], naccept [W], nswap [K][T-1], worst
        [K][T]); the counts run since begin."""
        T, counts, ndim = self._tmp_shape
        W = T * sum(counts)
        chain, llc, lprc = np.empty((nsteps, W, ndim)), np.empty((nsteps, W)), np.empty((nsteps, W))
        nacc, nswap, worst = np.zeros(W, dtype=np.int64), np.zeros((self.k, T - 1), dtype=np.int64), np.zeros((self.k, T), dtype=np.int32)
        self.check(self.lib.msx_group_tempered_collect(self.h, int(slot), dptr(chain), dptr(llc), dptr(lprc), iptr(nacc), iptr(nswap),
                                                       worst.ctypes.data_as(C.POINTER(C.c_int32))))
        return chain, llc, lprc, nacc, nswap, worst

    def tempered_end(self, want_state=False):
        """End the run (msx_group_tempered_end); its final (coords, ll, lpr) if want_state."""
        if not want_state:
            self.check(self.lib.msx_group_tempered_end(self.h, None, None, None))
            return None
        T, counts, ndim = self._tmp_shape
        W = T * sum(counts)
        coords, ll, lpr = np.empty((W, ndim)), np.empty(W), np.empty(W)
        self.check(self.lib.msx_group_tempered_end(self.h, dptr(coords), dptr(ll), dptr(lpr)))
        return coords, ll, lpr

    def tempered_attach_series(self, chain, dens, at_row):
        """Append every chunk of the run to the series ``chain`` (K T members, member k T + t of counts[k] walkers, ndim) and
        ``dens`` (the same members, ndim 2: ll, lpr) from row ``at_row`` on (msx_group_tempered_attach_series)."""
        self.check(self.lib.msx_group_tempered_attach_series(self.h, None if chain is None else chain.h, None if dens is None else dens.h,
                                                             int(at_row)))

    def tempered_adapt(self, lag, time, k0):
        """Make the run adaptive (msx_group_ladder_adapt): lag, time, k0 one per target; once, before the first enqueue."""
        lag, time, k0 = as_f64(lag), as_f64(time), np.ascontiguousarray(k0, dtype=np.int64)
        if lag.shape != (self.k,) or time.shape != (self.k,) or k0.shape != (self.k,):
            raise ValueError('tempered_adapt: lag, time and k0 one per target')
        self.check(self.lib.msx_group_ladder_adapt(self.h, dptr(lag), dptr(time), iptr(k0)))

    def tempered_betas(self, slot, nsteps):
        """(nsteps, K, T): the ladders the iterations of the chunk last collected from ``slot`` ran with (msx_group_ladder_betas)."""
        out = np.empty((int(nsteps), self.k, self._tmp_shape[0]))
        self.check(self.lib.msx_group_ladder_betas(self.h, int(slot), dptr(out)))
        return out

    def tempered_ladder(self):
        """(betas (K, T), k (K,), skipped (K,)): the ladders behind everything queued (msx_group_ladder_current; it waits)."""
        betas, k, skipped = np.empty((self.k, self._tmp_shape[0])), np.zeros(self.k, dtype=np.int64), np.zeros(self.k, dtype=np.int64)
        self.check(self.lib.msx_group_ladder_current(self.h, dptr(betas), iptr(k), iptr(skipped)))
        return betas, k, skipped


class Series:
    """One ``msx_series`` (include/msx.h): a chain of ``nw`` walkers x ``ndim`` kept on the device of ``ctx``, and its
    normalised autocorrelation.  ``counts``: the members' walker counts (a target group's, in member order); None for one."""

    def __init__(self, ctx, nw, ndim, counts=None, cap_hint=0):
        self.lib = load()
        counts = np.ascontiguousarray([nw] if counts is None else counts, dtype=np.int64)
        h = C.c_void_p()
        ctx.check(self.lib.msx_series_create(ctx.h, int(nw), int(ndim), counts.size, iptr(counts), int(cap_hint), C.byref(h)))
        self.h = h
        self.ctx = ctx   # (whoever makes a sibling series -- mcmc_spec_amd.reweight -- makes it on the same device)
        self.nw, self.ndim, self.k = int(nw), int(ndim), int(counts.size)
        self.counts = counts

    def close(self):
        if getattr(self, 'h', None):
            self.lib.msx_series_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def check(self, rc):
        if rc != MSX_OK:
            msg = self.lib.msx_series_last_error(self.h).decode()
            raise ValueError(msg) if rc == MSX_ERR_RANGE else MsxError(rc, msg)

    @property
    def rows(self):
        out = C.c_int64()
        self.check(self.lib.msx_series_rows(self.h, C.byref(out)))
        return out.value

    def append(self, rows):
        """Host rows (nrows, nw, ndim) appended."""
        rows = as_f64(rows)
        if rows.ndim != 3 or rows.shape[1:] != (self.nw, self.ndim):
            raise ValueError('append: rows must have shape (nrows, {}, {})'.format(self.nw, self.ndim))
        if rows.shape[0]:
            self.check(self.lib.msx_series_append(self.h, dptr(rows), rows.shape[0]))

    def read(self, row0=0, nrows=None):
        """Rows row0 .. row0 + nrows - 1 as (nrows, nw, ndim)."""
        nrows = self.rows - int(row0) if nrows is None else int(nrows)
        out = np.empty((nrows, self.nw, self.ndim))
        if nrows:
            self.check(self.lib.msx_series_read(self.h, int(row0), nrows, dptr(out)))
        return out

    def acf(self, n, discard=0, thin=1, lag0=0, nlag=None, dims=None):
        """f (k, ndim, nlag): the members' walker-averaged normalised autocorrelation at lags lag0 .. lag0 + nlag - 1 of
        rows[0:n][discard::thin] (msx_series_acf).  ``dims``: the dimensions to compute (others are NaN); None for all."""
        n_eff = len(range(int(discard), int(n), int(thin)))
        nlag = n_eff - int(lag0) if nlag is None else int(nlag)
        dims = range(self.ndim) if dims is None else dims
        mask = 0
        for d in dims:
            mask |= 1 << int(d)
        f = np.full((self.k, self.ndim, nlag), np.nan)
        self.check(self.lib.msx_series_acf(self.h, int(n), int(discard), int(thin), int(lag0), nlag, mask, dptr(f)))
        return f

    def evidence(self, n, discard=0, thin=1, col=0, db=None, nblocks=1):
        """(mean, lme), each (k, nblocks + 1): per member the mean of column ``col`` over rows[0:n][discard::thin] and all the
        member's walkers ([:, 0]) and over each of ``nblocks`` consecutive blocks of those rows ([:, 1:]), and
        ``ln mean exp(db[m] x)`` likewise -- None without ``db`` (k,).  msx_series_evidence: fixed summation order."""
        nblocks = int(nblocks)
        mean = np.empty((self.k, max(nblocks, 0) + 1))
        lme = None
        if db is not None:
            db = as_f64(db)
            if db.shape != (self.k,):
                raise ValueError('evidence: db needs one entry per member')
            lme = np.empty_like(mean)
        self.check(self.lib.msx_series_evidence(self.h, int(n), int(discard), int(thin), int(col), None if db is None else dptr(db), nblocks,
                                                dptr(mean), None if lme is None else dptr(lme)))
        return mean, lme

    def moments(self, n, discard=0, thin=1, cols=None, cov=True):
        """Split R-hat and the pooled moments of rows[0:n][discard::thin] (n' >= 4 rows), per member and column
        (msx_series_moments): {'within', 'var_plus', 'between', 'rhat', 'mean' (k, ncols), 'cov'
        (k, ncols, ncols) -- None without ``cov`` --, 'count' (k,) = n' W_m}.  ``rhat = sqrt(var_plus / within)`` is taken
        here; the rest are the device's numbers, in a summation order n' and the walker counts fix.  ``cols``: coordinates
        (None: all)."""
        cols = _col_codes(range(self.ndim) if cols is None else cols)
        nc = int(cols.size)
        within, var_plus, between, mean = (np.empty((self.k, nc)) for _ in range(4))
        cv = np.empty((self.k, nc, nc)) if cov else None
        self.check(self.lib.msx_series_moments(self.h, int(n), int(discard), int(thin), uptr(cols), nc, dptr(within), dptr(var_plus),
                                               dptr(between), dptr(mean), None if cv is None else dptr(cv)))
        with np.errstate(invalid='ignore', divide='ignore'):
            rhat = np.sqrt(var_plus / within)
        count = len(range(int(discard), int(n), int(thin))) * self.counts
        return {'within': within, 'var_plus': var_plus, 'between': between, 'rhat': rhat, 'mean': mean, 'cov': cv, 'count': count}

    def modes(self, n, discard, thin, cols, center, scale, ncomp, split_col, split_at, max_iter=50, tol=1e-10, ridge=1e-6):
        """The EM fits of msx_series_modes (``mcmc_spec_amd.modes`` is the definition) over
        rows[0:n][discard::thin]: ({'weight' (k, S, K), 'mean' (k, S, K, d), 'cov' (k, S, K, d, d), 'loglik', 'niter',
        'status' (k, S)}, nbad (k,)) in standardised units, components in start order.  ``center``, ``scale`` (k, d);
        ``split_col`` (S,) positions in ``cols``; ``split_at`` (k, S, K - 1) raw thresholds."""
        cols = _col_codes(cols)
        d, K = int(cols.size), int(ncomp)
        center, scale = as_f64(center), as_f64(scale)
        split_col = np.ascontiguousarray(split_col, dtype=np.int32).reshape(-1)
        S = int(split_col.size)
        split_at = as_f64(split_at)
        if center.shape != (self.k, d) or scale.shape != (self.k, d) or split_at.size != self.k * S * max(K - 1, 0):
            raise ValueError('modes: center and scale must have shape (k, ncols), split_at (k, nstarts, ncomp - 1)')
        i32p = C.POINTER(C.c_int32)
        Kc = max(K, 0)
        out = {'weight': np.empty((self.k, S, Kc)), 'mean': np.empty((self.k, S, Kc, d)), 'cov': np.empty((self.k, S, Kc, d, d)),
               'loglik': np.empty((self.k, S)), 'niter': np.zeros((self.k, S), dtype=np.int32),
               'status': np.zeros((self.k, S), dtype=np.int32)}
        nbad = np.zeros(self.k, dtype=np.int64)
        self.check(self.lib.msx_series_modes(self.h, int(n), int(discard), int(thin), uptr(cols), d, dptr(center), dptr(scale), K, S,
                                             split_col.ctypes.data_as(i32p), dptr(split_at) if split_at.size else None, int(max_iter),
                                             float(tol), float(ridge), dptr(out['weight']), dptr(out['mean']), dptr(out['cov']),
                                             dptr(out['loglik']), out['niter'].ctypes.data_as(i32p), out['status'].ctypes.data_as(i32p),
                                             iptr(nbad)))
        return out, nbad

    def mode_labels(self, n, discard, thin, cols, center, scale, weight, mean, cov, dst=None, want_labels=True):
        """(labels uint8 (n', nw) -- None without ``want_labels`` --, counts (k, K)) under one mixture per member
        (msx_series_mode_labels): ``weight`` (k, K), ``mean`` (k, K, d), ``cov`` (k, K, d, d) in standardised units.
        ``dst``: k * K series of one walker and this series' ndim, member-major; dst[m * K + j] is filled with member m's
        samples labelled j (all coordinates; walker ascending, then row ascending) and holds exactly counts[m, j] rows."""
        cols = _col_codes(cols)
        d = int(cols.size)
        center, scale, weight, mean, cov = (as_f64(a) for a in (center, scale, weight, mean, cov))
        K = int(weight.shape[-1]) if weight.ndim else 0
        if (center.shape != (self.k, d) or scale.shape != (self.k, d) or weight.shape != (self.k, K) or mean.shape != (self.k, K, d)
                or cov.shape != (self.k, K, d, d)):
            raise ValueError('mode_labels: center, scale (k, ncols); weight (k, K); mean (k, K, ncols); cov (k, K, ncols, ncols)')
        nrows = len(range(int(discard), int(n), int(thin)))
        labels = np.empty((max(nrows, 0), self.nw), dtype=np.uint8) if want_labels else None
        counts = np.zeros((self.k, K), dtype=np.int64)
        arr = None
        if dst is not None:
            dst = list(dst)
            if len(dst) != self.k * K:
                raise ValueError('mode_labels: one dst series per member and mode ({})'.format(self.k * K))
            arr = (C.c_void_p * len(dst))(*[s.h for s in dst])
        self.check(self.lib.msx_series_mode_labels(self.h, int(n), int(discard), int(thin), uptr(cols), d, dptr(center), dptr(scale), K,
                                                   dptr(weight), dptr(mean), dptr(cov),
                                                   None if labels is None else labels.ctypes.data_as(C.POINTER(C.c_uint8)),
                                                   iptr(counts), arr))
        return labels, counts

    def logprob(self, contexts, dst, mode=MODE_LOGPOST, row0=0, nrows=None):
        """Rows row0 .. row0 + nrows - 1 of this series scored once more: member m with ``contexts[m]``'s staged problem in
        ``mode`` (MODE_LOGPOST, MODE_LOGPRIOR or MODE_LOGLIKE), into the same rows of ``dst`` (ndim = 1, the same members;
        msx_series_logprob).  A rejected sample gives -inf, one with an error status NaN.  Returns the members' worst
        sample status (k,)."""
        contexts = list(contexts)
        if len(contexts) != self.k:
            raise ValueError('logprob: one context per member ({} members, {} contexts)'.format(self.k, len(contexts)))
        nrows = self.rows - int(row0) if nrows is None else int(nrows)
        arr = (C.c_void_p * self.k)(*[c.h for c in contexts])
        worst = np.zeros(self.k, dtype=np.int32)
        self.check(self.lib.msx_series_logprob(self.h, arr, int(mode), int(row0), nrows, dst.h, worst.ctypes.data_as(C.POINTER(C.c_int32))))
        return worst

    @staticmethod
    def lincomb(terms, dst, row0=0, nrows=None):
        """``dst[row][walker] = coef_0 * x_0 + coef_1 * x_1 + ...`` for ``terms`` = [(series, col, coef), ...] (1 .. 8 of
        them; NumPy's bits for that expression), rows row0 .. row0 + nrows - 1 (None: all the first term's series holds);
        ``dst`` has ndim = 1 and the terms' members (msx_series_lincomb)."""
        terms = list(terms)
        if not terms:
            raise ValueError('lincomb: at least one term (series, col, coef)')
        nrows = terms[0][0].rows - int(row0) if nrows is None else int(nrows)
        arr = (C.c_void_p * len(terms))(*[t[0].h for t in terms])
        cols = np.ascontiguousarray([int(t[1]) for t in terms], dtype=np.int32)
        coef = as_f64([float(t[2]) for t in terms])
        dst.check(dst.lib.msx_series_lincomb(len(terms), arr, cols.ctypes.data_as(C.POINTER(C.c_int32)), dptr(coef), int(row0), nrows, dst.h))

    def weights(self, n, w_dst, discard=0, thin=1):
        """This series (ndim = 1) read as log-weights: ``w = exp(logw - M_m)`` of rows [0, n) into ``w_dst`` (ndim = 1, the
        same members), M_m the member's largest value that is finite or -inf; NaN and +inf are bad and weigh 0
        (msx_series_weights).  Returns {'count', 'nbad', 'nzero' (k,) ints, 'sumw', 'sumw2', 'ess' (k,)} over
        rows[0:n][discard::thin]."""
        stats = np.empty((self.k, 6))
        self.check(self.lib.msx_series_weights(self.h, int(n), int(discard), int(thin), w_dst.h, dptr(stats)))
        out = {name: stats[:, i].astype(np.int64) for i, name in enumerate(('count', 'nbad', 'nzero'))}
        out.update(sumw=stats[:, 3].copy(), sumw2=stats[:, 4].copy(), ess=stats[:, 5].copy())
        return out

    def psis(self, n, tail_len, w_dst, lw_dst=None, discard=0, thin=1, want_tail=False):
        """This series (ndim = 1) read as log-weights and Pareto-smoothed over rows[0:n][discard::thin] (msx_series_psis):
        ``tail_len`` (k,) samples per member form the tail; the smoothed, max-normalised weights go to ``w_dst`` and the
        normalised log-weights to ``lw_dst`` (or None), both of ndim = 1 with the same members.  Returns {'khat' (k,), 'status'
        (k,), 'ntail' (k,), 'stats': ``weights``' dict for the smoothed weights, 'tail': with ``want_tail`` the tails' flat
        indices in (value, index) order, a list of k arrays}."""
        tail_len = np.ascontiguousarray(tail_len, dtype=np.int64).reshape(-1)
        if tail_len.size != self.k:
            raise ValueError('psis: one tail_len per member ({})'.format(self.k))
        khat, status, ntail, stats = np.empty(self.k), np.zeros(self.k, dtype=np.int32), np.zeros(self.k, dtype=np.int64), np.empty((self.k, 6))
        tail = np.zeros((self.k, PSIS_TAIL_MAX), dtype=np.int64) if want_tail else None
        self.check(self.lib.msx_series_psis(self.h, int(n), int(discard), int(thin), iptr(tail_len), w_dst.h, None if lw_dst is None else lw_dst.h,
                                            dptr(khat), status.ctypes.data_as(C.POINTER(C.c_int32)), iptr(ntail), dptr(stats),
                                            None if tail is None else iptr(tail)))
        st = {name: stats[:, i].astype(np.int64) for i, name in enumerate(('count', 'nbad', 'nzero'))}
        st.update(sumw=stats[:, 3].copy(), sumw2=stats[:, 4].copy(), ess=stats[:, 5].copy())
        out = {'khat': khat, 'status': status.astype(np.int64), 'ntail': ntail, 'stats': st}
        if want_tail:
            out['tail'] = [tail[m, :ntail[m]].copy() for m in range(self.k)]
        return out

    def wmoments(self, w, n, discard=0, thin=1, cols=None, cov=True):
        """{'sumw' (k,), 'mean' (k, ncols), 'cov' (k, ncols, ncols) or None}: the moments of rows[0:n][discard::thin] under
        the weights series ``w`` (msx_series_wmoments): mean = sum w x / sum w, cov = sum w (x - mean)(x - mean)^T / sum w."""
        cols = _col_codes(range(self.ndim) if cols is None else cols)
        nc = int(cols.size)
        sumw, mean = np.empty(self.k), np.empty((self.k, nc))
        cv = np.empty((self.k, nc, nc)) if cov else None
        self.check(self.lib.msx_series_wmoments(self.h, w.h, int(n), int(discard), int(thin), uptr(cols), nc, dptr(sumw), dptr(mean),
                                                None if cv is None else dptr(cv)))
        return {'sumw': sumw, 'mean': mean, 'cov': cv}

    def resample(self, w, n, nout, dst, discard=0, thin=1, seed=0):
        """Systematic resampling of rows[0:n][discard::thin] under the weights series ``w`` (msx_series_resample):
        ``dst[m]`` -- a series of one walker and this series' ndim -- receives member m's ``nout[m]`` drawn samples, all
        coordinates, and holds exactly that many rows.  Returns the drawn flat indices, a list of k int64 arrays."""
        nout = np.ascontiguousarray(nout, dtype=np.int64).reshape(-1)
        dst = list(dst)
        if nout.size != self.k or len(dst) != self.k:
            raise ValueError('resample: one nout and one dst series per member ({})'.format(self.k))
        arr = (C.c_void_p * self.k)(*[s.h for s in dst])
        idx = np.zeros(max(int(np.sum(np.maximum(nout, 0))), 1), dtype=np.int64)
        self.check(self.lib.msx_series_resample(self.h, w.h, int(n), int(discard), int(thin), int(seed) & 0xffffffffffffffff, iptr(nout),
                                                arr, iptr(idx)))
        cuts = np.concatenate([[0], np.cumsum(nout)])
        return [idx[cuts[m]:cuts[m + 1]].copy() for m in range(self.k)]

    def derive(self, contexts, cols, dst, row0=0, nrows=None):
        """Rows row0 .. row0 + nrows - 1 of this series mapped to the derived columns ``cols`` (codes) and written to the
        same rows of ``dst`` (ndim = len(cols), the same members); member m is evaluated with ``contexts[m]``
        (msx_series_derive).  Returns the members' worst sample status (k,)."""
        cols = _col_codes(cols)
        contexts = list(contexts)
        if len(contexts) != self.k:
            raise ValueError('derive: one context per member ({} members, {} contexts)'.format(self.k, len(contexts)))
        nrows = self.rows - int(row0) if nrows is None else int(nrows)
        arr = (C.c_void_p * self.k)(*[c.h for c in contexts])
        worst = np.zeros(self.k, dtype=np.int32)
        self.check(self.lib.msx_series_derive(self.h, arr, uptr(cols), cols.size, int(row0), nrows, dst.h,
                                              worst.ctypes.data_as(C.POINTER(C.c_int32))))
        return worst

    def predictive(self, contexts, npix, n, discard=0, thin=1, q=None, scratch_bytes=0, terms_dst=None):
        """msx_series_predictive over rows[0:n][discard::thin]: per member m, evaluated with ``contexts[m]`` whose problem
        has ``npix[m]`` pixels, the tuple (band (4, 1 + nspec, npix_m), quant (len(q), 1 + nspec, npix_m) or None, resid
        (3, npix_m)); then counts (k,) and the members' worst sample status (k,).  ``terms_dst``: a series of ndim 4 with the
        same members that receives the four chi^2 terms of every row 0 .. n - 1."""
        contexts = list(contexts)
        if len(contexts) != self.k or len(npix) != self.k:
            raise ValueError('predictive: one context and one pixel count per member ({} members)'.format(self.k))
        rows = self.ndim // 2   # 1 + nspec
        npix = [int(x) for x in npix]
        q = None if q is None else as_f64(np.atleast_1d(q))
        tot = sum(npix)
        band = np.empty(4 * rows * tot)
        quant = None if q is None else np.empty(q.size * rows * tot)
        resid = np.empty(3 * tot)
        count = np.zeros(self.k, dtype=np.int64)
        worst = np.zeros(self.k, dtype=np.int32)
        arr = (C.c_void_p * self.k)(*[c.h for c in contexts])
        self.check(self.lib.msx_series_predictive(self.h, arr, int(n), int(discard), int(thin), None if q is None else dptr(q),
                                                  0 if q is None else q.size, int(scratch_bytes), dptr(band),
                                                  None if quant is None else dptr(quant), dptr(resid),
                                                  None if terms_dst is None else terms_dst.h, iptr(count),
                                                  worst.ctypes.data_as(C.POINTER(C.c_int32))))
        out, off = [], 0
        for m in range(self.k):
            b = band[4 * rows * off:4 * rows * (off + npix[m])].reshape(4, rows, npix[m])
            qq = None if quant is None else quant[q.size * rows * off:q.size * rows * (off + npix[m])].reshape(q.size, rows, npix[m])
            out.append((b, qq, resid[3 * off:3 * (off + npix[m])].reshape(3, npix[m])))
            off += npix[m]
        return out, count, worst

    def pointwise(self, contexts, n, discard=0, thin=1, reff=1.0, scratch_bytes=0, want_matrix=False):
        """msx_series_pointwise over rows[0:n][discard::thin]: per member m, evaluated with ``contexts[m]``, the tuple (out (6,
        n_obs_m), the pointwise matrix (n_obs_m, count_m) or None); then counts, tail lengths and the members' worst sample
        status, each (k,)."""
        contexts = list(contexts)
        if len(contexts) != self.k:
            raise ValueError('pointwise: one context per member ({} members)'.format(self.k))
        nobs = [sum(c.pointwise_nobs()) for c in contexts]
        nsel = len(range(int(discard), int(n), int(thin))) * np.asarray(self.counts, dtype=np.int64) if int(thin) >= 1 else np.zeros(self.k, dtype=np.int64)
        out = np.empty(6 * sum(nobs))
        slots = [int(nobs[m] * nsel[m]) for m in range(self.k)]
        ll = np.empty(max(sum(slots), 1)) if want_matrix else None
        count, tail, worst = np.zeros(self.k, dtype=np.int64), np.zeros(self.k, dtype=np.int64), np.zeros(self.k, dtype=np.int32)
        arr = (C.c_void_p * self.k)(*[c.h for c in contexts])
        self.check(self.lib.msx_series_pointwise(self.h, arr, int(n), int(discard), int(thin), float(reff), int(scratch_bytes), dptr(out),
                                                 iptr(count), iptr(tail), worst.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 None if ll is None else dptr(ll)))
        parts, o, l = [], 0, 0
        for m in range(self.k):
            mat = None if ll is None else ll[l:l + nobs[m] * int(count[m])].reshape(nobs[m], int(count[m])).copy()
            parts.append((out[o:o + 6 * nobs[m]].reshape(6, nobs[m]), mat))
            o += 6 * nobs[m]
            l += slots[m]
        return parts, count, tail, worst

    # ---- the split pool, transformed: rank-normalised R-hat, bulk / tail ESS, MCSE ----------------
    def split_sibling(self, ncols):
        """An empty series for ``split_transform``'s results: 2 nw walkers, members of 2 W_m, ``ncols`` columns."""
        return Series(self.ctx, 2 * self.nw, int(ncols), 2 * self.counts)

    def split_transform(self, n, discard, thin, cols, transform, dst, param=None, scratch_bytes=0):
        """The split pool of rows[0:n][discard::thin] (n' >= 4 rows), transformed, into ``dst`` (``split_sibling``), which then
        holds h = n' // 2 rows: half-chain 2 w + half of walker w is walker 2 w + half of dst (msx_series_split_transform).
        ``transform``: SPLIT_IDENTITY, SPLIT_RANKNORM, SPLIT_FOLD_RANKNORM (``param`` (k, ncols): the medians), SPLIT_INDICATOR
        (``param``: the thresholds) or SPLIT_RANK2 (twice the average rank).  ``cols``: coordinates or ``col_ratio`` codes.
        ``scratch_bytes``: the sort's budget (0: 256 MiB); the result does not depend on it."""
        cols = _col_codes(cols)
        if param is not None:
            param = as_f64(param)
            if param.shape != (self.k, cols.size):
                raise ValueError('split_transform: param must have shape (k, ncols)')
        self.check(self.lib.msx_series_split_transform(self.h, int(n), int(discard), int(thin), uptr(cols), cols.size, int(transform),
                                                       None if param is None else dptr(param), int(scratch_bytes), dst.h))

    def chain_acov(self, n, lag0=0, nlag=None, cols=None):
        """(A (k, ncols, nlag), mean_var (k, ncols), between (k, ncols)) of rows[0:n] with every walker a chain
        (msx_series_chain_acov): the chain-averaged biased autocovariance at lags lag0 .. lag0 + nlag - 1, A(0) n / (n - 1) and
        the variance (ddof 1) of the chains' means."""
        cols = _col_codes(range(self.ndim) if cols is None else cols)
        nlag = int(n) - int(lag0) if nlag is None else int(nlag)
        A = np.empty((self.k, cols.size, max(nlag, 0)))
        mv, bt = np.empty((self.k, cols.size)), np.empty((self.k, cols.size))
        self.check(self.lib.msx_series_chain_acov(self.h, int(n), int(lag0), nlag, uptr(cols), cols.size, dptr(A), dptr(mv), dptr(bt)))
        return A, mv, bt

    def chain_ess(self, n, lag_tile=320):
        """{'ess', 'rhat', 'mean_var', 'between', 'max_t'}, each (k, ndim), of rows[0:n] with every walker a chain: Geyer's
        sequences (``diagnostics.geyer_tau``) over lag tiles of ``lag_tile``, 2 ``lag_tile``, ... asked for until every column's
        sequence has ended -- the loop is sequential, so an end found in a prefix is the end the full length gives -- and the
        plain R-hat of the chains, sqrt(((n - 1) / n mean_var + between) / mean_var)."""
        from . import diagnostics
        n, k, nd = int(n), self.k, self.ndim
        S = n * self.counts
        ess, max_t = np.full((k, nd), np.nan), np.zeros((k, nd), dtype=np.int64)
        mv, bt = np.empty((k, nd)), np.empty((k, nd))
        prefix = np.empty((k, nd, 0))
        pending = {(m, d) for m in range(k) for d in range(nd)}
        lag0, tile = 0, int(lag_tile)
        while pending:
            nlag = min(tile, n - lag0)
            cols = sorted({d for _, d in pending})
            A, v, b = self.chain_acov(n, lag0, nlag, cols)
            full = np.full((k, nd, nlag), np.nan)
            full[:, cols] = A
            prefix = np.concatenate([prefix, full], axis=2)
            if lag0 == 0:
                mv, bt = v, b
            lag0 += nlag
            tile *= 2
            for m, d in sorted(pending):
                tau, cut = diagnostics.geyer_tau(prefix[m, d], mv[m, d], bt[m, d], n, int(S[m]))
                if tau is None:
                    continue
                ess[m, d], max_t[m, d] = S[m] / tau, cut
                pending.discard((m, d))
        with np.errstate(invalid='ignore', divide='ignore'):
            rhat = np.sqrt(((n - 1) / n * mv + bt) / mv)
        return {'ess': ess, 'rhat': rhat, 'mean_var': mv, 'between': bt, 'max_t': max_t}

    def rank_stats(self, n, discard=0, thin=1, cols=None, q=(0.16, 0.5, 0.84), want=('rhat', 'bulk', 'tail', 'mean', 'mcse'),
                   scratch_bytes=0, lag_tile=320):
        """``diagnostics.rank_rhat`` / ``ess`` / ``mcse`` of rows[0:n][discard::thin] (n' >= 4 rows) per member and column, from
        the series itself: the split pool's transforms (``split_transform``) go to two sibling series, their autocovariances
        come back in lag tiles (``chain_ess``), the pool's median and quantiles are exact order statistics of the IDENTITY
        series, and Geyer's loop, the maxima, the Beta quantiles and the square roots are the host's.  -> a dict of (k, ncols)
        arrays, as ``want`` names them: 'rhat' -> 'bulk', 'folded', 'rhat'; 'bulk' / 'tail' / 'mean' -> 'ess_bulk' / 'ess_tail'
        / 'ess_mean'; 'mcse' -> 'mcse_mean', 'ess_quantile' and 'mcse_quantile' (k, ncols, len(q)).  A column with a non-finite
        value or one distinct value is NaN everywhere."""
        from . import diagnostics, summary
        cols = list(range(self.ndim)) if cols is None else [int(c) for c in np.atleast_1d(cols)]
        q = [float(p) for p in np.atleast_1d(q)] if 'mcse' in want else []
        if any(not 0.0 < p < 1.0 for p in q):
            raise ValueError('every q must lie in (0, 1)')
        nc, h = len(cols), len(range(int(discard), int(n), int(thin))) // 2
        if h < 2:
            raise ValueError('chain too short')
        S = 2 * h * self.counts
        out = {}
        ident, work = self.split_sibling(nc), self.split_sibling(nc)
        try:
            def ess_of(transform, param=None):
                self.split_transform(n, discard, thin, cols, transform, work, param, scratch_bytes)
                return work.chain_ess(h, lag_tile)
            self.split_transform(n, discard, thin, cols, SPLIT_IDENTITY, ident)
            pool = summary.summary_of(ident, h, [0.05, 0.95] + q)
            # NaN sorts last and the infinities to the ends: the pool's extremes say whether it has an answer at all
            bad = ~(np.isfinite(pool['min']) & np.isfinite(pool['max'])) | (pool['min'] == pool['max'])
            z = ess_of(SPLIT_RANKNORM) if 'rhat' in want or 'bulk' in want else None
            if 'rhat' in want:
                self.split_transform(n, discard, thin, cols, SPLIT_FOLD_RANKNORM, work, pool['median'], scratch_bytes)
                _, mv, bt = work.chain_acov(h, 0, 1)
                with np.errstate(invalid='ignore', divide='ignore'):
                    out['bulk'], out['folded'] = z['rhat'], np.sqrt(((h - 1) / h * mv + bt) / mv)
                    out['rhat'] = np.maximum(out['bulk'], out['folded'])
            if 'bulk' in want:
                out['ess_bulk'] = z['ess']
            if 'tail' in want:
                lo, hi = (ess_of(SPLIT_INDICATOR, pool['quantiles'][:, :, i])['ess'] for i in (0, 1))
                with np.errstate(invalid='ignore'):
                    out['ess_tail'] = np.minimum(lo, hi)
            if 'mean' in want or 'mcse' in want:
                x = ident.chain_ess(h, lag_tile)
                out['ess_mean'] = x['ess']
            if 'mcse' in want:
                J = 2 * self.counts[:, None]
                with np.errstate(invalid='ignore', divide='ignore'):
                    # the pooled variance (ddof 1) from the chains' own: sum_j sum_i (x - m_j)^2 + h sum_j (m_j - mbar)^2
                    var = ((J * (h - 1)) * x['mean_var'] + (h * (J - 1)) * x['between']) / (S[:, None] - 1)
                    out['mcse_mean'] = np.sqrt(var) / np.sqrt(x['ess'])
                out['ess_quantile'] = np.full((self.k, nc, len(q)), np.nan)
                ranks = np.zeros((self.k, nc, len(q), 2), dtype=np.int64)
                for i, p in enumerate(q):
                    e = ess_of(SPLIT_INDICATOR, pool['quantiles'][:, :, 2 + i])['ess']
                    out['ess_quantile'][:, :, i] = e
                    for m, c in np.ndindex(self.k, nc):
                        if np.isfinite(e[m, c]):
                            ranks[m, c, i] = diagnostics.mcse_quantile_of(lambda r: 0.0, int(S[m]), e[m, c], p)[1]
                out['mcse_quantile'] = np.full((self.k, nc, len(q)), np.nan)
                if q:
                    vals, _ = ident.order_stats(h, 0, 1, range(nc), ranks.reshape(self.k, -1))
                    for m, c, i in np.ndindex(self.k, nc, len(q)):
                        th1, th2 = vals[m, c].reshape(nc, len(q), 2)[c, i]
                        if np.isfinite(out['ess_quantile'][m, c, i]):
                            out['mcse_quantile'][m, c, i] = (th2 - th1) / 2.0
        finally:
            ident.close()
            work.close()
        for name, v in out.items():
            if name != 'max_t':
                v[bad] = np.nan
        return out

    def order_stats(self, n, discard, thin, cols, ranks):
        """(values (k, ncols, nranks), counts (k,)): the elements of zero-based ranks ``ranks`` (k, nranks; one row is
        used for every member) in ascending order of each member's flat sample rows[0:n][discard::thin] of each column
        (msx_series_order_stats; np.sort's order, NaN last).  ``cols``: coordinates or ``col_ratio(a, b)`` codes."""
        cols = _col_codes(cols)
        ranks = np.atleast_2d(np.asarray(ranks, dtype=np.int64))
        if ranks.ndim != 2 or ranks.shape[0] not in (1, self.k) or ranks.shape[1] < 1 or cols.size < 1:
            raise ValueError('order_stats: ranks must have shape (k, nranks), nranks >= 1, and cols must name a column')
        ranks = np.ascontiguousarray(np.broadcast_to(ranks, (self.k, ranks.shape[1])))
        out = np.empty((self.k, cols.size, ranks.shape[1]))
        count = np.zeros(self.k, dtype=np.int64)
        self.check(self.lib.msx_series_order_stats(self.h, int(n), int(discard), int(thin), uptr(cols), cols.size, iptr(ranks),
                                                   ranks.shape[1], dptr(out), iptr(count)))
        return out, count

    def hist(self, n, discard, thin, cols, edges, closed_last=True):
        """int64 counts (k, ncols, nedges - 1) of each member's column against its own ascending edge vector, ``edges``
        (k, ncols, nedges): bin b holds edges[b] <= x < edges[b + 1]; the last edge itself counts in the last bin when
        ``closed_last`` (np.histogram) and nowhere otherwise (the reference's loop).  msx_series_hist."""
        cols = _col_codes(cols)
        edges = as_f64(edges)
        if edges.ndim != 3 or edges.shape[:2] != (self.k, cols.size):
            raise ValueError('hist: edges must have shape (k, ncols, nedges)')
        counts = np.zeros((self.k, cols.size, max(edges.shape[2] - 1, 0)), dtype=np.int64)
        self.check(self.lib.msx_series_hist(self.h, int(n), int(discard), int(thin), uptr(cols), cols.size, dptr(edges),
                                            edges.shape[2], int(bool(closed_last)), iptr(counts)))
        return counts

    def hist2d(self, n, discard, thin, pairs, xedges, yedges, closed_last=True):
        """int64 counts (k, npairs, nx - 1, ny - 1) for the column pairs ``pairs`` (npairs, 2) = (cx, cy), with ``xedges``
        (k, npairs, nx) and ``yedges`` (k, npairs, ny); hist's edge rule on both axes, at most 128 bins each
        (msx_series_hist2d; np.histogram2d with closed_last)."""
        pairs = np.ascontiguousarray(np.asarray(pairs, dtype=np.int64).reshape(-1, 2).astype(np.uint32))
        xedges, yedges = as_f64(xedges), as_f64(yedges)
        npairs = pairs.shape[0]
        if xedges.ndim != 3 or yedges.ndim != 3 or xedges.shape[:2] != (self.k, npairs) or yedges.shape[:2] != (self.k, npairs):
            raise ValueError('hist2d: xedges and yedges must have shape (k, npairs, nedges)')
        counts = np.zeros((self.k, npairs, max(xedges.shape[2] - 1, 0), max(yedges.shape[2] - 1, 0)), dtype=np.int64)
        self.check(self.lib.msx_series_hist2d(self.h, int(n), int(discard), int(thin), uptr(pairs), npairs, dptr(xedges),
                                              xedges.shape[2], dptr(yedges), yedges.shape[2], int(bool(closed_last)), iptr(counts)))
        return counts


# ---- the device-resident samplers' marshalling, shared by Context (msx_sampler_*) and Group (msx_group_sampler_*) ----
def _sampler_enqueue(owner, fn, half, slot, arrays):
    """fn(h, slot, nsteps, sidx, cidx, partner, zz, zfac, logu) for one chunk of arrays (nsteps, 2, owner's walkers / 2);
    ``half`` names that size in the error message."""
    i32p = C.POINTER(C.c_int32)
    arrs = [np.ascontiguousarray(a, dtype=np.int32) for a in arrays[:3]]
    dbl = [as_f64(a) for a in arrays[3:]]
    nsteps = dbl[0].shape[0]
    for a in arrs + dbl:
        if a.shape != (nsteps, 2, owner._smp_shape[0] // 2):
            raise ValueError('sampler_enqueue: arrays must have shape (nsteps, 2, {})'.format(half))
    owner.check(fn(owner.h, int(slot), nsteps, arrs[0].ctypes.data_as(i32p), arrs[1].ctypes.data_as(i32p),
                   arrs[2].ctypes.data_as(i32p), dptr(dbl[0]), dptr(dbl[1]), dptr(dbl[2])))
    return nsteps


def _move_set(moves):
    """``moves`` (a MsxMoveSet, or anything the samplers' ``moves=`` takes) as msx_move_set."""
    if isinstance(moves, MsxMoveSet):
        return moves
    from .moves import parse_moves
    return parse_moves(moves).as_struct()


def _sampler_enqueue_moves(owner, fn, k, slot, arrays):
    """fn(h, slot, nsteps, sidx, cidx, kind, p1, p2, g, fac, logu) for one chunk in the general layout: kind (nsteps,) for
    one ensemble or (nsteps, k), the others (nsteps, 2, owner's walkers / 2)."""
    i32p = C.POINTER(C.c_int32)
    sidx, cidx, kind, p1, p2 = (np.ascontiguousarray(a, dtype=np.int32) for a in arrays[:5])
    dbl = [as_f64(a) for a in arrays[5:]]
    nsteps = dbl[0].shape[0]
    for a in [sidx, cidx, p1, p2] + dbl:
        if a.shape != (nsteps, 2, owner._smp_shape[0] // 2):
            raise ValueError('sampler_enqueue_moves: arrays must have shape (nsteps, 2, walkers / 2)')
    if kind.size != nsteps * k:
        raise ValueError('sampler_enqueue_moves: kind must have one entry per iteration and member')
    owner.check(fn(owner.h, int(slot), nsteps, *[a.ctypes.data_as(i32p) for a in (sidx, cidx, kind, p1, p2)], dptr(dbl[0]), dptr(dbl[1]),
                   dptr(dbl[2])))
    return nsteps


def _collect_out(shape, nsteps):
    """A chunk's outputs for the run's (walkers, ndim): chain [nsteps][n][ndim], logp [nsteps][n], naccept [n]."""
    n, ndim = shape
    return np.empty((nsteps, n, ndim)), np.empty((nsteps, n)), np.zeros(n, dtype=np.int64)


def _sampler_end(owner, fn, want_state):
    """fn(h, coords, logp): end the run; its final (coords, logp) if want_state."""
    if not want_state:
        owner.check(fn(owner.h, None, None))
        return None
    n, ndim = owner._smp_shape
    coords, logp = np.empty((n, ndim)), np.empty(n)
    owner.check(fn(owner.h, dptr(coords), dptr(logp)))
    return coords, logp


def ladder_step(betas, counts, nw, k, lag, time):
    """``(betas', skipped)`` of one ladder step through the library's host entry (msx_ladder_step): the C text the adapt kernel
    runs, with no context and no GPU.  ``mcmc_spec_amd.tempered.ladder_step`` is the definition it must equal bit for bit."""
    betas = as_f64(betas).reshape(-1)
    counts = np.ascontiguousarray(counts, dtype=np.int64).reshape(-1)
    if len(counts) != max(len(betas) - 1, 0):
        raise ValueError('ladder_step: one count per adjacent pair')
    out, skipped = np.empty(len(betas)), C.c_int32(0)
    rc = load().msx_ladder_step(len(betas), dptr(betas), iptr(counts), int(nw), int(k), float(lag), float(time), dptr(out), C.byref(skipped))
    if rc != MSX_OK:
        raise ValueError('msx_ladder_step refused its arguments (code {})'.format(rc))
    return out, int(skipped.value)
