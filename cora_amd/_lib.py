"""ctypes binding of libcorahip.so (include/corahip.h) + a thin torch-tensor front end.

PyTorch is used for device memory, streams and (elsewhere) torch.distributed only;
all arithmetic of the hot path runs in the hand-written HIP kernels of the library.
There is NO CPU fallback: if the library or a gfx950 GPU is missing, the compute
entry points raise (loudly) instead of computing something else.
"""
import ctypes
import os
import weakref

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("CORAHIP_LIB", os.path.join(_HERE, "libcorahip.so"))  # override: diagnostics only

c_int, c_double, c_void_p, c_size_t = ctypes.c_int, ctypes.c_double, ctypes.c_void_p, ctypes.c_size_t
c_u64, c_char_p = ctypes.c_uint64, ctypes.c_char_p
PTR = c_void_p

# name -> (restype, argtypes): every symbol include/corahip.h declares
SIGNATURES = {
    "corahip_abi_version": (c_int, []),
    "corahip_abi_minor": (c_int, []),
    "corahip_last_error": (c_char_p, []),
    "corahip_device_count": (c_int, [ctypes.POINTER(c_int)]),
    "corahip_ctx_create": (c_int, [c_int, ctypes.POINTER(c_void_p)]),
    "corahip_ctx_destroy": (c_int, [c_void_p]),
    "corahip_ctx_set_stream": (c_int, [c_void_p, c_void_p]),
    "corahip_ctx_sync": (c_int, [c_void_p]),
    "corahip_timer_begin": (c_int, [c_void_p]),
    "corahip_timer_end": (c_int, [c_void_p, ctypes.POINTER(ctypes.c_float)]),
    "corahip_profile_enable": (c_int, [c_void_p, c_int]),
    "corahip_profile_get": (c_int, [c_void_p, c_char_p, ctypes.POINTER(c_double), ctypes.POINTER(c_int)]),
    "corahip_profile_reset": (c_int, [c_void_p]),
    "corahip_malloc": (c_int, [c_void_p, c_size_t, ctypes.POINTER(c_void_p)]),
    "corahip_free": (c_int, [c_void_p, c_void_p]),
    "corahip_memcpy_h2d": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    "corahip_memcpy_d2h": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    "corahip_clarray_table21cm": (c_int, [c_void_p, PTR, PTR, PTR, c_int, c_int, c_double, c_double, c_double,
                                          PTR, PTR, PTR, PTR, c_int, c_int, PTR, PTR, c_int, PTR]),
    "corahip_clarray_table21cm_pairs": (c_int, [c_void_p, PTR, PTR, PTR, c_int, c_int, c_double, c_double, c_double,
                                                PTR, PTR, PTR, PTR, c_int, c_int, PTR, PTR, c_int, c_int, c_int, c_int,
                                                PTR]),
    "corahip_clarray_pairs_finish": (c_int, [c_void_p, PTR, c_int, c_int, c_int, c_int, PTR]),
    "corahip_clarray_tables_pin": (c_int, [c_void_p, PTR, PTR, PTR, c_u64]),
    "corahip_aps_table21cm_points": (c_int, [c_void_p, PTR, PTR, PTR, c_int, c_int, c_double, c_double, c_double,
                                             ctypes.c_long, PTR, PTR, PTR, PTR, PTR, PTR, PTR]),
    "corahip_clarray_separable": (c_int, [c_void_p, PTR, c_int, PTR, c_int, c_int, PTR, PTR]),
    "corahip_romb_reduce": (c_int, [c_void_p, PTR, c_int, c_int, c_int, PTR, PTR]),
    "corahip_factor_batched": (c_int, [c_void_p, PTR, c_int, c_int, c_double, c_double, PTR, PTR]),
    "corahip_normals_philox": (c_int, [c_void_p, c_u64, c_int, c_int, PTR]),
    "corahip_normals_pcg64": (c_int, [c_void_p, ctypes.POINTER(c_u64), ctypes.POINTER(c_u64), ctypes.c_int64, PTR,
                                      ctypes.POINTER(c_u64)]),
    "corahip_normal_rows_pcg64": (c_int, [c_void_p, ctypes.POINTER(c_u64), ctypes.POINTER(c_u64), ctypes.c_long, ctypes.c_long,
                                          PTR, PTR, PTR, c_int, ctypes.POINTER(c_u64)]),
    "corahip_normals_mt19937_legacy": (c_int, [c_void_p, c_void_p, ctypes.c_int64, PTR]),
    "corahip_glibc_exp": (c_int, [c_void_p, PTR, ctypes.c_int64, PTR]),
    "corahip_pcg64_advance": (c_int, [ctypes.POINTER(c_u64), ctypes.POINTER(c_u64), c_u64, ctypes.POINTER(c_u64)]),
    "corahip_draw_alm_philox": (c_int, [c_void_p, PTR, PTR, c_u64, c_int, c_int, c_int, c_int, PTR]),
    "corahip_draw_alm_philox_rows": (c_int, [c_void_p, PTR, PTR, c_u64, c_int, c_int, c_int, c_int, PTR]),
    "corahip_draw_alm": (c_int, [c_void_p, PTR, PTR, PTR, c_int, c_int, c_int, c_int, PTR]),
    "corahip_draw_alm_rows": (c_int, [c_void_p, PTR, PTR, PTR, c_int, c_int, c_int, c_int, PTR]),
    "corahip_draw_alm_numpy_prepare": (c_int, [c_void_p, c_void_p, c_int, c_int, c_size_t, ctypes.POINTER(c_void_p)]),
    "corahip_draw_alm_numpy_run": (c_int, [c_void_p, c_void_p, PTR, c_int, PTR, c_void_p, PTR]),
    "corahip_draw_alm_numpy": (c_int, [c_void_p, PTR, c_int, PTR, c_void_p, c_int, c_int, c_int, c_int, PTR, c_size_t]),
    "corahip_draw_alm_numpy_begin": (c_int, [c_void_p, PTR, c_int, PTR, c_void_p, c_int, c_int, c_int, c_int, PTR, c_size_t,
                                             ctypes.POINTER(c_void_p)]),
    "corahip_draw_alm_numpy_end": (c_int, [c_void_p, c_void_p, c_void_p]),
    "corahip_draw_alm_numpy_begin_set": (c_int, [c_void_p, PTR, PTR, c_void_p, c_int, c_int, c_void_p, PTR, c_size_t,
                                                 ctypes.POINTER(c_void_p)]),
    "corahip_draw_alm_philox_rows_set": (c_int, [c_void_p, PTR, PTR, c_u64, c_int, c_int, c_void_p, PTR]),
    "corahip_mkfullsky_workspace_bytes": (c_int, [c_void_p, c_int, c_int, c_int, c_int, c_int, ctypes.POINTER(c_size_t)]),
    "corahip_mkfullsky": (c_int, [c_void_p, c_void_p, PTR, c_int, c_void_p, c_int, c_int, c_int, PTR, c_void_p, c_size_t]),
    "corahip_shard_plan": (c_int, [c_int, c_int, c_int, c_int, PTR]),
    "corahip_factor_rows_pack": (c_int, [c_void_p, PTR, c_int, c_int, c_int, c_int, PTR]),
    "corahip_factor_rows_unpack": (c_int, [c_void_p, PTR, PTR, c_int, c_int, c_int, c_int, PTR]),
    "corahip_alm_dev_to_square": (c_int, [c_void_p, PTR, c_int, c_int, PTR]),
    "corahip_alm_packed_to_dev": (c_int, [c_void_p, PTR, c_int, c_int, PTR]),
    "corahip_sht_plan_create": (c_int, [c_void_p, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "corahip_sht_plan_create_ex": (c_int, [c_void_p, c_int, c_int, c_int, ctypes.POINTER(c_void_p)]),
    "corahip_sht_plan_cut_exp": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "corahip_sht_plan_k4_mfma_count": (c_int, [c_void_p, c_void_p, c_int, ctypes.POINTER(c_u64)]),
    "corahip_sht_plan_destroy": (c_int, [c_void_p, c_void_p]),
    "corahip_alm2map_workspace_bytes": (c_int, [c_void_p, c_int, ctypes.POINTER(c_size_t)]),
    "corahip_alm2map": (c_int, [c_void_p, c_void_p, PTR, c_int, PTR, c_void_p, c_size_t]),
    "corahip_map2alm_workspace_bytes": (c_int, [c_void_p, c_int, ctypes.POINTER(c_size_t)]),
    "corahip_map2alm": (c_int, [c_void_p, c_void_p, PTR, c_int, PTR, PTR, c_void_p, c_size_t]),
    "corahip_alm2map_spin2": (c_int, [c_void_p, c_void_p, PTR, c_int, PTR, c_void_p, c_size_t]),
    "corahip_spin2_ring_scale": (c_int, [c_void_p, c_void_p, PTR, c_int, PTR]),
    "corahip_spin2_combine": (c_int, [c_void_p, c_void_p, PTR, c_int, c_int, PTR, c_int]),
    "corahip_map2alm_spin2_workspace_bytes": (c_int, [c_void_p, c_int, ctypes.POINTER(c_size_t)]),
    "corahip_map2alm_spin2": (c_int, [c_void_p, c_void_p, PTR, c_int, PTR, PTR, c_void_p, c_size_t]),
    "corahip_xi_table_max_knots": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "corahip_xi_table_average": (c_int, [c_void_p, PTR, PTR, PTR, c_int, c_int, c_double, c_double, PTR, c_int, PTR, PTR,
                                         c_int, c_int, PTR]),
    "corahip_ps_table21cm": (c_int, [c_void_p, PTR, PTR, PTR, c_int, c_int, c_double, PTR, c_int, PTR, c_int, c_double,
                                     PTR, PTR, PTR, PTR]),
    "corahip_dct1_workspace_bytes": (c_int, [ctypes.c_long, c_int, ctypes.POINTER(c_size_t)]),
    "corahip_dct1_rows": (c_int, [c_void_p, PTR, ctypes.c_long, c_int, c_double, c_void_p, c_size_t]),
    "corahip_legendre_project": (c_int, [c_void_p, PTR, PTR, c_int, c_int, PTR, ctypes.c_long, PTR]),
    "corahip_xi_multi_average": (c_int, [c_void_p, PTR, PTR, PTR, c_int, c_int, c_int, c_double,
                                         ctypes.POINTER(c_double), PTR, c_int, PTR, PTR, c_int, c_int, c_int, PTR]),
    "corahip_cl_blocks": (c_int, [c_void_p, PTR, ctypes.c_long, c_int, c_int, PTR]),
    "corahip_fft_c2c": (c_int, [c_void_p, PTR, c_int, PTR, c_int, c_int]),
    "corahip_irfftn": (c_int, [c_void_p, PTR, c_int, PTR, c_int, PTR]),
    "corahip_rfftn": (c_int, [c_void_p, PTR, c_int, PTR, c_int, PTR]),
    "corahip_randomfield_draw": (c_int, [c_void_p, PTR, ctypes.c_int64, ctypes.c_uint64, PTR]),
    "corahip_fg_mix": (c_int, [c_void_p, PTR, PTR, PTR, c_int, c_int, ctypes.c_int64, PTR]),
    "corahip_randomfield_irfftn": (c_int, [c_void_p, PTR, c_int, PTR, ctypes.c_uint64, PTR, PTR]),
    "corahip_spec_mul_real": (c_int, [c_void_p, PTR, PTR, ctypes.c_int64]),
    "corahip_cube_affine": (c_int, [c_void_p, PTR, PTR, PTR, PTR, PTR, c_int, ctypes.c_int64, PTR]),
    "corahip_raytrace_slices": (c_int, [c_void_p, PTR, c_int, c_int, c_int, PTR, PTR, PTR, PTR, c_double, c_double,
                                        c_int, c_int, c_int, PTR]),
    "corahip_healpix_neighbours": (c_int, [c_void_p, c_int, PTR]),
    "corahip_za_density_sph": (c_int, [c_void_p, PTR, PTR, PTR, PTR, c_int, c_int, c_double, c_double, PTR]),
    "corahip_der1_alm_prep": (c_int, [c_void_p, c_void_p, PTR, c_int, c_int, c_int, PTR]),
    "corahip_der1_combine": (c_int, [c_void_p, c_void_p, PTR, c_int, c_int, PTR, PTR, c_int, PTR, PTR]),
    "corahip_radial_gradient": (c_int, [c_void_p, PTR, PTR, PTR, c_int, ctypes.c_long, PTR]),
    "corahip_slice_mix": (c_int, [c_void_p, PTR, PTR, PTR, c_int, ctypes.c_long, PTR]),
    "corahip_slice_diff2": (c_int, [c_void_p, PTR, PTR, PTR, PTR, PTR, PTR, c_int, ctypes.c_long, PTR]),
    "corahip_slice_moments_workspace_bytes": (c_int, [c_int, ctypes.c_long, ctypes.POINTER(c_size_t)]),
    "corahip_slice_moments": (c_int, [c_void_p, PTR, ctypes.c_long, PTR, c_int, ctypes.c_long, c_void_p, c_size_t, PTR,
                                      PTR]),
    "corahip_bias_field": (c_int, [c_void_p, PTR, PTR, PTR, PTR, c_int, ctypes.c_long, PTR]),
    "corahip_lognormal": (c_int, [c_void_p, PTR, PTR, PTR, c_double, c_int, ctypes.c_long, ctypes.c_long, PTR]),
    "corahip_alm_cross_spectra": (c_int, [c_void_p, PTR, c_int, PTR, c_int, c_int, PTR]),
    "corahip_alm_gather_channels": (c_int, [c_void_p, PTR, c_int, PTR, c_int, c_int, PTR, c_int, c_int]),
    "corahip_healpix_interp_weights": (c_int, [c_void_p, c_int, PTR, PTR, ctypes.c_long, PTR, PTR]),
    "corahip_healpix_interp_val": (c_int, [c_void_p, PTR, ctypes.c_long, c_int, PTR, PTR, ctypes.c_long, PTR]),
    "corahip_healpix_rotate_maps": (c_int, [c_void_p, PTR, ctypes.c_long, c_int, ctypes.POINTER(c_double), PTR]),
    "corahip_za_density_grid": (c_int, [c_void_p, PTR, PTR, PTR, c_int, c_int, PTR]),
    "corahip_complex_variance": (c_int, [c_void_p, PTR, ctypes.c_long, PTR]),
    "corahip_faraday_mix": (c_int, [c_void_p, PTR, ctypes.c_long, c_int, PTR, PTR, PTR, c_int, c_double, PTR, PTR]),
    "corahip_faraday_pack": (c_int, [c_void_p, PTR, c_int, ctypes.c_long, c_int, c_int, PTR]),
    "corahip_pointsource_population": (c_int, [c_void_p, c_u64, ctypes.c_long, PTR, PTR, PTR, c_int, c_double, c_double,
                                               c_double, ctypes.c_long, PTR, PTR, PTR, PTR, PTR]),
    "corahip_pointsource_paint": (c_int, [c_void_p, ctypes.c_long, PTR, PTR, PTR, PTR, PTR, PTR, PTR, c_double, c_int, c_int,
                                          ctypes.c_long, c_int, PTR]),
    "corahip_polarise_rotate": (c_int, [c_void_p, PTR, PTR, PTR, PTR, PTR, c_int, ctypes.c_long, PTR]),
    "corahip_faraday_rotate": (c_int, [c_void_p, PTR, PTR, PTR, c_int, c_int, ctypes.c_long]),
    "corahip_healpix_ud_grade": (c_int, [c_void_p, PTR, ctypes.c_long, c_int, c_int, PTR]),
    "corahip_healpix_reorder": (c_int, [c_void_p, PTR, ctypes.c_long, c_int, c_int, PTR]),
    "corahip_healpix_block_variance": (c_int, [c_void_p, PTR, ctypes.c_long, c_int, c_int, PTR]),
    "corahip_alm_scale_l": (c_int, [c_void_p, PTR, c_int, c_int, PTR, PTR]),
    "corahip_galaxy_combine": (c_int, [c_void_p, PTR, PTR, PTR, PTR, PTR, c_double, PTR, c_int, c_int, ctypes.c_long, PTR]),
    "corahip_eig_top_max_f": (c_int, [c_void_p, ctypes.POINTER(c_int)]),
    "corahip_eig_top_batched": (c_int, [c_void_p, PTR, c_int, c_int, c_int, c_int, PTR, PTR, PTR]),
    "corahip_constrained_weights": (c_int, [c_void_p, PTR, c_int, c_int, c_int, PTR, PTR, PTR]),
    "corahip_alm_mix_l": (c_int, [c_void_p, PTR, c_int, c_int, PTR, c_int, PTR]),
    "corahip_sinc_romb": (c_int, [c_void_p, PTR, PTR, c_int, c_double, PTR, c_int, PTR]),
    "corahip_fftlog_phase": (c_int, [c_void_p, c_double, c_double, ctypes.c_int64, PTR]),
    "corahip_jl_romb": (c_int, [c_void_p, PTR, c_int, ctypes.POINTER(c_int), PTR, c_int, c_double, PTR, c_int, PTR]),
    "corahip_xi_rsd": (c_int, [c_void_p, PTR, PTR, PTR, c_int, c_int, PTR, PTR, ctypes.c_long, PTR, ctypes.c_long, PTR]),
    "corahip_powerlaw_los": (c_int, [c_void_p, PTR, PTR, PTR, c_double, c_double, c_double, c_double, c_int, ctypes.c_long, c_int,
                                     PTR]),
    "corahip_field_moments": (c_int, [c_void_p, PTR, ctypes.c_long, c_int, PTR]),
    "corahip_sphbessel_radial": (c_int, [c_void_p, PTR, c_int, PTR, PTR, PTR, c_int, c_int, c_int, ctypes.c_long, PTR]),
    "corahip_cl_gram": (c_int, [c_void_p, PTR, PTR, c_int, c_int, c_int, ctypes.c_long, PTR, c_int]),
    "corahip_clarray_fullsky_workspace_bytes": (c_int, [c_int, c_int, c_int, ctypes.POINTER(c_size_t)]),
    "corahip_clarray_fullsky": (c_int, [c_void_p, PTR, PTR, c_int, PTR, PTR, PTR, c_int, c_int, c_int, c_int, PTR, PTR]),
    "corahip_logconv": (c_int, [c_void_p, PTR, PTR, ctypes.c_int64, c_int, c_int]),
    "corahip_logconv_split": (c_int, [ctypes.c_int64, ctypes.POINTER(c_int), ctypes.POINTER(c_int)]),
    "corahip_sht_plan_rings": (c_int, [c_void_p, PTR, PTR, PTR, PTR]),
    "corahip_sht_plan_ring_classes": (c_int, [c_void_p, PTR]),
    "corahip_sht_lambda": (c_int, [c_void_p, c_void_p, c_int, c_int, PTR]),
    "corahip_sht_lambda_entry": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, PTR]),
    "corahip_sht_lambda_segment_entry": (c_int, [c_void_p, c_void_p, c_int, c_int, c_int, c_int, PTR, PTR]),
    "corahip_debug_poison_scratch": (c_int, [c_void_p, c_int, ctypes.POINTER(c_size_t)]),
}

DEBUG_NSCRATCH = 13          # include/corahip.h: CORAHIP_DEBUG_NSCRATCH, the scratch slots of a context


class CoraHipError(RuntimeError):
    """An entry point of libcorahip.so returned a non-zero status (``status``: <0 a CORAHIP_E* code of include/corahip.h,
    >0 a hipError_t)."""

    status = 0


CORAHIP_ESTATE = -3          # include/corahip.h: an object used in the wrong state (e.g. a second draw session on a context)

_lib = None


def load():
    """Load libcorahip.so and attach prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "cora_amd: %s not found. Build it with `make -C cora_amd/csrc` (needs hipcc, gfx950). "
                "There is no CPU fallback for the compute path." % LIB_PATH
            )
        # torch bundles its own libamdhip64.so.7; import it FIRST so that libcorahip.so binds to the
        # same HIP runtime instance (streams and device pointers are shared with torch).  Loading
        # the library first would pull in /opt/rocm's copy and leave two runtimes in the process.
        try:
            import torch  # noqa: F401
        except ImportError:
            pass
        lib = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(lib, name)
            fn.restype = res
            fn.argtypes = args
        if lib.corahip_abi_version() != 1:
            raise ImportError("cora_amd: ABI version mismatch in %s" % LIB_PATH)
        _lib = lib
    return _lib


def pcg64_advance(state, inc, delta):
    """PCG64 state (python int) after ``delta`` steps - numpy's ``bit_generator.advance`` as host arithmetic of the
    library (no GPU needed)."""
    M = 2**64 - 1
    st = (c_u64 * 2)((int(state) >> 64) & M, int(state) & M)
    ic = (c_u64 * 2)((int(inc) >> 64) & M, int(inc) & M)
    out = (c_u64 * 2)()
    _check(load().corahip_pcg64_advance(st, ic, c_u64(int(delta)), out))
    return (int(out[0]) << 64) | int(out[1])


def _check(rc):
    if rc != 0:
        msg = load().corahip_last_error()
        err = CoraHipError("libcorahip status %d: %s" % (rc, msg.decode() if msg else "?"))
        err.status = int(rc)
        raise err


def _torch():
    import torch

    return torch


class _MtState(ctypes.Structure):          # corahip_mt_state
    _fields_ = [("key", ctypes.c_uint32 * 624), ("pos", ctypes.c_int32), ("has_gauss", ctypes.c_int32), ("gauss", c_double)]


class _Rng(ctypes.Structure):              # corahip_rng
    _fields_ = [("kind", ctypes.c_int32), ("reserved", ctypes.c_int32), ("stream", c_void_p), ("seed", c_u64),
                ("state", c_u64 * 2), ("inc", c_u64 * 2), ("legacy", ctypes.POINTER(_MtState))]


class _ChanSet(ctypes.Structure):          # corahip_chanset
    _fields_ = [("nchunks", ctypes.c_int32), ("chunk_nnu", ctypes.c_int32), ("nu0", ctypes.c_int32 * 2)]


def _chanset(chunks):
    """[(first channel, count)] (one block, or the two equal chunks of a folded shard) -> corahip_chanset."""
    cs = _ChanSet()
    chunks = [(int(a), int(n)) for a, n in chunks]
    if len(chunks) not in (1, 2) or (len(chunks) == 2 and chunks[0][1] != chunks[1][1]):
        raise ValueError("a channel set is one block or two equal chunks")
    cs.nchunks, cs.chunk_nnu = len(chunks), chunks[0][1]
    cs.nu0[0] = chunks[0][0]
    cs.nu0[1] = chunks[1][0] if len(chunks) == 2 else 0
    return cs


def _rng_struct(rng):
    """("pcg64", state, inc) | ("legacy", state dict) -> (corahip_rng, corahip_mt_state or None)."""
    r = _Rng()
    M = 2**64 - 1
    if rng[0] == "pcg64":
        r.kind = 2
        r.state[0], r.state[1] = (int(rng[1]) >> 64) & M, int(rng[1]) & M
        r.inc[0], r.inc[1] = (int(rng[2]) >> 64) & M, int(rng[2]) & M
        return r, None
    if rng[0] != "legacy" or rng[1]["bit_generator"] != "MT19937":
        raise ValueError("numpy stream on the device: ('pcg64', state, inc) or ('legacy', MT19937 state dict)")
    ms = _mt_struct(rng[1])
    r.kind = 3
    r.legacy = ctypes.pointer(ms)
    return r, ms


def _mt_struct(state):
    """``get_state(legacy=False)`` of a legacy generator on MT19937 -> corahip_mt_state."""
    if state["bit_generator"] != "MT19937":
        raise ValueError("legacy stream on the device: MT19937 only")
    ms = _MtState()
    key = np.ascontiguousarray(state["state"]["key"], dtype=np.uint32)
    ctypes.memmove(ms.key, key.ctypes.data, 624 * 4)
    ms.pos, ms.has_gauss, ms.gauss = int(state["state"]["pos"]), int(state["has_gauss"]), float(state["gauss"])
    return ms


def _mt_dict(ms):
    """corahip_mt_state -> the dict ``set_state`` takes."""
    return {"bit_generator": "MT19937", "state": {"key": np.frombuffer(ms.key, dtype=np.uint32).copy(), "pos": int(ms.pos)},
            "has_gauss": int(ms.has_gauss), "gauss": float(ms.gauss)}


class DrawSession:
    """One draw with numpy's own stream on a context: ``corahip_draw_alm_numpy_prepare`` (here) -> :meth:`run` (``_run``:
    K3 against the factors) -> :meth:`finish` (``_end``: the one read-back).  The session holds what the library reads
    until then (the ``corahip_rng`` struct, the MT state it points to, the tensors of the run) and is the one place that
    ends the C session: ``_end`` is called exactly once - by ``finish``, by :meth:`abort`, by ``run`` when it raises, or
    by the finalizer of a session that was dropped - and a session that did not run whole leaves the generator untouched."""

    def __init__(self, ctx, rng, lmax, F, ring_bytes=0):
        self.rng_struct, self.mt_state = _rng_struct(rng)
        self.shape, self.state, self.keep = (int(lmax), int(F)), "prepared", []
        pend = c_void_p()
        _check(ctx.lib.corahip_draw_alm_numpy_prepare(ctx.h, ctypes.byref(self.rng_struct), int(lmax), int(F), int(ring_bytes),
                                                      ctypes.byref(pend)))
        self.ctx, self.pending = ctx, pend
        # (the callback keeps the struct and the MT state alive, not the session; nothing is ended at interpreter exit)
        self._end = weakref.finalize(self, lambda r, ms: ctx.lib.corahip_draw_alm_numpy_end(ctx.h, pend, ctypes.byref(r)),
                                     self.rng_struct, self.mt_state)
        self._end.atexit = False

    def run(self, T, info, lmax, F, nu0=0, nnu=None, out=None, rows=False, chunks=None):
        """K3 of every range against ``T`` (arguments as :meth:`Context.draw_alm_numpy`); returns the a_lm.  Whatever is
        raised here - a shape that does not fit, the allocation of the a_lm, a status of the library - ends the session."""
        ctx = self.ctx
        try:
            assert self.state == "prepared" and self.shape == (int(lmax), int(F)), "the prepared session is for another shape"
            if chunks is not None:
                rows, nu0, nnu = True, chunks[0][0], sum(c[1] for c in chunks)
            nnu = F if nnu is None else nnu
            assert tuple(T.shape) == ((lmax + 1, nnu, F) if rows else (lmax + 1, F, F)), T.shape
            alm = ctx._alm_out(lmax, nnu, out)
            cs = _chanset(chunks if chunks is not None and len(chunks) > 1 else [(nu0, nnu)])
            _check(ctx.lib.corahip_draw_alm_numpy_run(ctx.h, self.pending, ctx._f64(T), 1 if rows else 0, ctx._p0(info),
                                                      ctypes.byref(cs), ctx._f64(alm)))
        except BaseException:
            self.state = "ended"
            self._end()
            raise
        self.state, self.keep = "ran", [T, info, alm]           # (alive until the queue has been waited for)
        return alm

    def finish(self):
        """``corahip_draw_alm_numpy_end`` behind a run: waits for the queue; returns the generator's state after - the
        PCG64 state as a python int, or the legacy state dict ``set_state`` takes."""
        assert self.state == "ran", self.state
        self.state = "ended"
        rc = self._end()
        self.keep = []
        _check(rc)
        if self.mt_state is not None:
            return _mt_dict(self.mt_state)
        return (int(self.rng_struct.state[0]) << 64) | int(self.rng_struct.state[1])

    def abort(self):
        """Give up a session that has not finished (generator untouched); harmless on one that has ended."""
        if self._end.alive:
            self.state, self.keep = "ended", []
            _check(self._end())


class Context:
    """One context per GPU; wraps the C ABI with torch tensors as device arrays."""

    def __init__(self, device=0):
        torch = _torch()
        self.lib = load()
        if not torch.cuda.is_available():
            raise CoraHipError(
                "cora_amd needs an AMD MI355X (gfx950) GPU: torch.cuda.is_available() is False "
                "and there is no CPU fallback"
            )
        self.device = torch.device("cuda", device)
        torch.cuda.set_device(self.device)
        h = c_void_p()
        _check(self.lib.corahip_ctx_create(device, ctypes.byref(h)))
        self.h = h
        self._plans = {}
        self._workspace = None
        self.use_current_stream()

    # -- plumbing ---------------------------------------------------------------------
    def use_current_stream(self):
        torch = _torch()
        s = torch.cuda.current_stream(self.device).cuda_stream
        _check(self.lib.corahip_ctx_set_stream(self.h, c_void_p(s)))

    def sync(self):
        _check(self.lib.corahip_ctx_sync(self.h))

    def timer_begin(self):
        _check(self.lib.corahip_timer_begin(self.h))

    def timer_end(self):
        ms = ctypes.c_float()
        _check(self.lib.corahip_timer_end(self.h, ctypes.byref(ms)))
        return float(ms.value)

    def profile_enable(self, on=True):
        _check(self.lib.corahip_profile_enable(self.h, 1 if on else 0))

    def profile_reset(self):
        _check(self.lib.corahip_profile_reset(self.h))

    def profile_get(self, name):
        ms, n = c_double(), c_int()
        _check(self.lib.corahip_profile_get(self.h, name.encode(), ctypes.byref(ms), ctypes.byref(n)))
        return float(ms.value), int(n.value)

    def empty(self, shape, dtype=None):
        torch = _torch()
        return torch.empty(shape, dtype=dtype or torch.float64, device=self.device)

    def to_device(self, a, dtype=np.float64):
        torch = _torch()
        a = np.ascontiguousarray(a, dtype=dtype)
        return torch.from_numpy(a).to(self.device)

    @staticmethod
    def _p(t):
        assert t.is_contiguous(), "device array must be contiguous"
        return c_void_p(t.data_ptr())

    def _f64(self, t):
        torch = _torch()
        assert t.dtype == torch.float64 and t.device == self.device
        return self._p(t)

    def _p0(self, t):
        return self._p(t) if t is not None else None

    def _alm_out(self, lmax, nnu, out=None):
        """``out``, or a fresh a_lm buffer in the device layout [nalm, ceil(nnu / 4), 2, 4]."""
        return out if out is not None else self.empty(((lmax + 1) * (lmax + 2) // 2, (nnu + 3) // 4, 2, 4))

    # -- host delivery ------------------------------------------------------------------
    _PINNED_MIN_BYTES = 1 << 24     # below this a pageable copy is as fast as pinning a buffer

    @property
    def copy_stream(self):
        """A second HIP stream for host <-> device copies that overlap the kernels of the library's stream."""
        torch = _torch()
        if getattr(self, "_copy_stream", None) is None:
            self._copy_stream = torch.cuda.Stream(device=self.device)
        return self._copy_stream

    def to_host_async(self, t):
        """Start the D2H copy of device tensor ``t`` into PINNED host memory on the copy stream (after everything
        queued so far on the current stream); returns ``(host_tensor, event)``.  The pinned block comes from torch's
        caching host allocator: the first buffer of a size is page-locked once (seconds for tens of GB), later ones of
        that size are recycled as soon as the caller drops the array."""
        torch = _torch()
        host = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
        ready = torch.cuda.Event()
        ready.record(torch.cuda.current_stream(self.device))
        cs = self.copy_stream
        cs.wait_event(ready)
        with torch.cuda.stream(cs):
            host.copy_(t, non_blocking=True)
            done = torch.cuda.Event()
            done.record(cs)
        t.record_stream(cs)
        return host, done

    def to_host(self, t):
        """Device tensor -> numpy array.  Large arrays arrive through pinned memory at PCIe rate (the ndarray is a view
        of the pinned block and keeps it alive); small ones by an ordinary pageable copy."""
        if t.numel() * t.element_size() < self._PINNED_MIN_BYTES:
            return t.cpu().numpy()
        host, done = self.to_host_async(t)
        done.synchronize()
        return host.numpy()

    # -- K1 ---------------------------------------------------------------------------
    def pin_tables(self, dd, dv, vv, generation):
        """The 21cm tables (dd, dv, vv) stay as they are under this generation number: K1 keeps its transposed copy
        of them between calls (corahip_clarray_tables_pin).  The model that owns the tables calls this."""
        _check(self.lib.corahip_clarray_tables_pin(self.h, self._f64(dd), self._f64(dv), self._f64(vv), c_u64(int(generation))))

    def unpin_tables(self, generation=0):
        """Withdraws the pin of ``generation`` (0: whatever is pinned): the owner calls this before its tables are
        freed or replaced - a recycled device address must never be taken for the pinned tables."""
        if self.h:
            _check(self.lib.corahip_clarray_tables_pin(self.h, None, None, None, c_u64(int(generation))))

    def clarray_table21cm(self, dd, dv, vv, kperpmin, kperpmax, kparmax, chi, pfd, f, b, F, zint, w, log10l):
        nl = log10l.numel()
        out = self.empty((nl, F, F))
        nkperp, nkpar = dd.shape
        _check(self.lib.corahip_clarray_table21cm(
            self.h, self._f64(dd), self._f64(dv), self._f64(vv), nkperp, nkpar, kperpmin, kperpmax, kparmax,
            self._f64(chi), self._f64(pfd), self._f64(f), self._f64(b), F, zint, self._f64(w), self._f64(log10l),
            nl, self._f64(out)))
        return out

    def clarray_table21cm_pairs(self, dd, dv, vv, kperpmin, kperpmax, kparmax, chi, pfd, f, b, F, zint, w, log10l,
                                pair_first, pair_step, l_block, nblocks=None):
        """Pair shard of the integration: [nblocks >= ceil(nl / l_block), npl, l_block] slabs (see
        include/corahip.h); nblocks = number of ranks when the slabs feed an all-to-all."""
        torch = _torch()
        nl = log10l.numel()
        npl = (F * (F + 1) // 2 + pair_step - 1) // pair_step
        nblk = (nl + l_block - 1) // l_block
        if nblocks is not None:
            assert nblocks >= nblk
            nblk = nblocks
        out = torch.zeros((nblk, npl, l_block), dtype=torch.float64, device=self.device)
        nkperp, nkpar = dd.shape
        _check(self.lib.corahip_clarray_table21cm_pairs(
            self.h, self._f64(dd), self._f64(dv), self._f64(vv), nkperp, nkpar, kperpmin, kperpmax, kparmax,
            self._f64(chi), self._f64(pfd), self._f64(f), self._f64(b), F, zint, self._f64(w), self._f64(log10l),
            nl, pair_first, pair_step, l_block, self._f64(out)))
        return out

    def clarray_pairs_finish(self, slabs, F, nl):
        """[nranks, npl, l_stride] pair slabs (slab r integrated by rank r) -> C [nl, F, F]."""
        nranks, npl, l_stride = slabs.shape
        assert npl == (F * (F + 1) // 2 + nranks - 1) // nranks and nl <= l_stride
        out = self.empty((nl, F, F))
        _check(self.lib.corahip_clarray_pairs_finish(self.h, self._f64(slabs), F, nranks, l_stride, nl, self._f64(out)))
        return out

    def aps_table21cm_points(self, dd, dv, vv, kperpmin, kperpmax, kparmax, lx, chi1, chi2, cdd, cdv, cvv):
        n = lx.numel()
        out = self.empty((n,))
        nkperp, nkpar = dd.shape
        _check(self.lib.corahip_aps_table21cm_points(
            self.h, self._f64(dd), self._f64(dv), self._f64(vv), nkperp, nkpar, kperpmin, kperpmax, kparmax, n,
            self._f64(lx), self._f64(chi1), self._f64(chi2), self._f64(cdd), self._f64(cdv), self._f64(cvv),
            self._f64(out)))
        return out

    def clarray_separable(self, al, bcov, F, zint, w):
        nl = al.numel()
        out = self.empty((nl, F, F))
        _check(self.lib.corahip_clarray_separable(self.h, self._f64(al), nl, self._f64(bcov), F, zint,
                                                  self._f64(w), self._f64(out)))
        return out

    def romb_reduce(self, clt, nl, F, zint, w):
        out = self.empty((nl, F, F))
        _check(self.lib.corahip_romb_reduce(self.h, self._f64(clt), nl, F, zint, self._f64(w), self._f64(out)))
        return out

    # -- K0 ---------------------------------------------------------------------------
    def ps_table21cm(self, kperp, kpar, spline=None, kstar=0.0, freq_window=0.0, dd=None):
        """(dd, dv, vv) device tables [nkperp, nkpar] BEFORE the DCT: from a spline description
        ``spline = (loglog, x, y, y2)`` (device arrays) or from a host-evaluated ``dd`` (device array)."""
        nkperp, nkpar = kperp.numel(), kpar.numel()
        dv, vv = self.empty((nkperp, nkpar)), self.empty((nkperp, nkpar))
        if dd is None:
            loglog, kx, ky, ky2 = spline
            dd = self.empty((nkperp, nkpar))
            _check(self.lib.corahip_ps_table21cm(self.h, self._f64(kx), self._f64(ky), self._f64(ky2), kx.numel(),
                                                 1 if loglog else 0, float(kstar), self._f64(kperp), nkperp,
                                                 self._f64(kpar), nkpar, float(freq_window), None, self._f64(dd),
                                                 self._f64(dv), self._f64(vv)))
        else:
            _check(self.lib.corahip_ps_table21cm(self.h, None, None, None, 0, 0, 0.0, self._f64(kperp), nkperp,
                                                 self._f64(kpar), nkpar, 0.0, self._f64(dd), None, self._f64(dv),
                                                 self._f64(vv)))
        return dd, dv, vv

    def dct1_rows(self, data, scale=1.0):
        """In place: every row of the device array ``data`` [nrows, n] -> scipy.fftpack.dct(row, type=1) * scale."""
        nrows, n = data.shape
        b = c_size_t()
        _check(self.lib.corahip_dct1_workspace_bytes(nrows, n, ctypes.byref(b)))
        ws = self.workspace(int(b.value))
        _check(self.lib.corahip_dct1_rows(self.h, self._f64(data), nrows, n, float(scale), self._p(ws), int(b.value)))
        return data

    # -- K2 ---------------------------------------------------------------------------
    def factor_batched(self, C, jitter_rel=1e-14, eig_thresh=1e-16):
        torch = _torch()
        nl, F, F2 = C.shape
        assert F == F2
        T = self.empty((nl, F, F))
        info = torch.empty((nl,), dtype=torch.int32, device=self.device)
        _check(self.lib.corahip_factor_batched(self.h, self._f64(C), nl, F, jitter_rel, eig_thresh, self._f64(T),
                                               self._p(info)))
        return T, info

    # -- K3 ---------------------------------------------------------------------------
    def normals_philox(self, seed, lmax, F, out=None):
        n = 2 * F * (lmax + 1) * (lmax + 2) // 2
        g = out if out is not None else self.empty((n,))
        assert g.numel() >= n
        _check(self.lib.corahip_normals_philox(self.h, c_u64(int(seed) & (2**64 - 1)), lmax, F, self._f64(g)))
        return g

    def normals_pcg64(self, state, inc, n, out=None):
        """The next ``n`` values of numpy's ``Generator(PCG64).standard_normal`` from bit-generator ``state`` / ``inc``
        (python ints, 128 bits), generated on the device; returns (g, n_raw): the normals and the number of raw 64-bit
        draws they consumed (see :func:`pcg64_advance`)."""
        g = out if out is not None else self.empty((n,))
        assert g.numel() >= n
        M = 2**64 - 1
        st = (c_u64 * 2)((int(state) >> 64) & M, int(state) & M)
        ic = (c_u64 * 2)((int(inc) >> 64) & M, int(inc) & M)
        nraw = c_u64(0)
        _check(self.lib.corahip_normals_pcg64(self.h, st, ic, int(n), self._f64(g), ctypes.byref(nraw)))
        return g, int(nraw.value)

    @staticmethod
    def check_rows(scale, ncol, out, row_off=None):
        """The host-side argument checks of :meth:`normal_rows_pcg64` (no device call): ``scale`` [nrow], ``out`` a
        contiguous float64 tensor, every row ``row_off[r] : row_off[r] + ncol`` (``row_off`` None: ``r * ncol``) inside
        ``out`` - ValueError otherwise.  Returns ``(nrow, row_off as a host int64 array or None)``."""
        torch = _torch()
        if len(scale.shape) != 1:
            raise ValueError("scale must be one value per row (got shape %s)" % (tuple(scale.shape),))
        nrow = int(scale.shape[0])
        if ncol < 0:
            raise ValueError("ncol must not be negative (got %d)" % ncol)
        if not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float64 tensor")
        size = int(out.numel())
        if row_off is None:
            if nrow * ncol > size:
                raise ValueError("out holds %d values, %d rows of %d need %d" % (size, nrow, ncol, nrow * ncol))
            return nrow, None
        ro = row_off.cpu().numpy() if isinstance(row_off, torch.Tensor) else np.asarray(row_off)
        if ro.shape != (nrow,) or ro.dtype.kind not in "iu":
            raise ValueError("row_off must be %d integers (got shape %s, dtype %s)" % (nrow, ro.shape, ro.dtype))
        ro = np.ascontiguousarray(ro, dtype=np.int64)
        bad = np.flatnonzero((ro < 0) | (ro > size - ncol))
        if len(bad):
            raise ValueError("row_off[%d] = %d: a row of %d values from there would leave out (%d values)"
                             % (int(bad[0]), int(ro[bad[0]]), ncol, size))
        return nrow, ro

    def normal_rows_pcg64(self, state, inc, scale, ncol, out, row_off=None, accumulate=False):
        """numpy's ``Generator(PCG64).normal(scale=scale[:, None], size=(len(scale), ncol))`` from bit-generator
        ``state`` / ``inc`` (python ints), written (``accumulate=False``) or added (``True``) in place on the device:
        row ``r`` goes to ``out.view(-1)[row_off[r] : row_off[r] + ncol]`` (``row_off`` None: ``r * ncol``).  ``scale``:
        [nrow] host array or device tensor; ``row_off``: [nrow] integers (host array or device tensor), rows must not
        overlap; ``out``: a contiguous device float64 tensor.  Every ``row_off[r] + ncol`` is checked against ``out``
        here, on the host (:meth:`check_rows`, ValueError) - the kernel cannot.  Returns ``n_raw``, the raw draws
        consumed."""
        torch = _torch()
        ncol = int(ncol)
        sc = scale.to(dtype=torch.float64).contiguous() if isinstance(scale, torch.Tensor) \
            else np.ascontiguousarray(scale, dtype=np.float64)
        nrow, ro = self.check_rows(sc, ncol, out, row_off)
        if nrow == 0 or ncol == 0:
            return 0
        if not isinstance(sc, torch.Tensor):
            sc = self.to_device(sc)
        if ro is not None:
            ro = self.to_device(ro, dtype=np.int64)
        M = 2**64 - 1
        st = (c_u64 * 2)((int(state) >> 64) & M, int(state) & M)
        ic = (c_u64 * 2)((int(inc) >> 64) & M, int(inc) & M)
        nraw = c_u64(0)
        _check(self.lib.corahip_normal_rows_pcg64(self.h, st, ic, nrow, ncol, self._f64(sc), self._p0(ro), self._f64(out),
                                                  1 if accumulate else 0, ctypes.byref(nraw)))
        return int(nraw.value)

    def glibc_exp(self, x):
        """exp(x) of a device float64 tensor as the wedge test of the device ziggurat evaluates it (glibc's routine,
        restated): the test hook ``corahip_glibc_exp``."""
        y = self.empty(tuple(x.shape))
        _check(self.lib.corahip_glibc_exp(self.h, self._f64(x), int(x.numel()), self._f64(y)))
        return y

    def normals_legacy(self, state, n, out=None):
        """The next ``n`` values of numpy's LEGACY stream (``np.random.standard_normal`` / ``RandomState``: MT19937 + polar
        method) from ``state`` = ``get_state(legacy=False)``, generated on the device; returns (g, state after) with the
        state as a dict ``set_state`` takes."""
        ms = _mt_struct(state)
        g = out if out is not None else self.empty((n,))
        assert g.numel() >= n
        _check(self.lib.corahip_normals_mt19937_legacy(self.h, ctypes.byref(ms), int(n), self._f64(g)))
        return g, _mt_dict(ms)

    def draw_alm(self, T, info, g, lmax, F, nu0=0, nnu=None, out=None):
        nnu = F if nnu is None else nnu
        alm = self._alm_out(lmax, nnu, out)
        _check(self.lib.corahip_draw_alm(self.h, self._f64(T), self._p0(info),
                                         self._f64(g), lmax, F, nu0, nnu, self._f64(alm)))
        return alm

    def draw_alm_rows(self, T_rows, info, g, lmax, F, nu0, nnu, out=None):
        """draw_alm with T_rows [lmax+1, nnu, F] = rows nu0..nu0+nnu-1 of every factor."""
        assert tuple(T_rows.shape) == (lmax + 1, nnu, F), T_rows.shape
        alm = self._alm_out(lmax, nnu, out)
        _check(self.lib.corahip_draw_alm_rows(self.h, self._f64(T_rows), self._p0(info),
                                              self._f64(g), lmax, F, nu0, nnu, self._f64(alm)))
        return alm

    def draw_alm_numpy_prepare(self, rng, lmax, F, ring_bytes=0):
        """``corahip_draw_alm_numpy_prepare``: the generator's part of :meth:`draw_alm_numpy` - its count / jump passes and
        the first two ranges of normals - enqueued on the library's generator stream NOW, so that it runs beside
        whatever the caller enqueues next (the kernels that make the factors).  Returns the :class:`DrawSession`
        ``draw_alm_numpy`` takes as ``prepared``; its ``abort()`` gives the session up (generator untouched)."""
        return DrawSession(self, rng, lmax, F, ring_bytes)

    def draw_alm_numpy(self, T, info, rng, lmax, F, nu0=0, nnu=None, out=None, rows=False, ring_bytes=0, defer=False,
                       chunks=None, prepared=None):
        """``corahip_draw_alm_numpy``: K3 with numpy's own stream generated on the device range by range (no 16 F nalm
        byte buffer).  ``rng``: ("pcg64", state, inc) python ints of a PCG64 bit generator, or ("legacy",
        get_state(legacy=False) dict).  ``rows``: T is the row block [L, nnu, F].  Returns (alm, state after): the PCG64
        state as a python int, or the legacy state dict ``set_state`` takes.  ``defer``: returns (alm, finish) instead -
        everything is enqueued, nothing waited for; ``finish()`` (``corahip_draw_alm_numpy_end``: the one read-back)
        returns the state after and is called once the caller has enqueued what follows (the synthesis).
        ``chunks``: [(first, count), (first, count)] - the two chunks of a folded frequency shard (row-block T in local
        channel order) instead of ``nu0`` / ``nnu``.  ``prepared``: the session of :meth:`draw_alm_numpy_prepare` (``rng``
        and ``ring_bytes`` are then ignored: the session carries the generator); without it the session is made here."""
        session = prepared if prepared is not None else self.draw_alm_numpy_prepare(rng, lmax, F, ring_bytes)
        alm = session.run(T, info, lmax, F, nu0=nu0, nnu=nnu, out=out, rows=rows, chunks=chunks)
        return (alm, session.finish) if defer else (alm, session.finish())

    def draw_alm_philox(self, T, info, seed, lmax, F, nu0=0, nnu=None, out=None):
        nnu = F if nnu is None else nnu
        alm = self._alm_out(lmax, nnu, out)
        _check(self.lib.corahip_draw_alm_philox(self.h, self._f64(T), self._p0(info),
                                                c_u64(int(seed) & (2**64 - 1)), lmax, F, nu0, nnu, self._f64(alm)))
        return alm

    def draw_alm_philox_rows(self, T_rows, info, seed, lmax, F, nu0, nnu, out=None):
        """draw_alm_philox with T_rows [lmax+1, nnu, F] = rows nu0..nu0+nnu-1 of every factor."""
        assert tuple(T_rows.shape) == (lmax + 1, nnu, F), T_rows.shape
        alm = self._alm_out(lmax, nnu, out)
        _check(self.lib.corahip_draw_alm_philox_rows(self.h, self._f64(T_rows), self._p0(info),
                                                     c_u64(int(seed) & (2**64 - 1)), lmax, F, nu0, nnu, self._f64(alm)))
        return alm

    def draw_alm_philox_chunks(self, T_rows, info, seed, lmax, F, chunks, out=None):
        """draw_alm_philox_rows for the channels of ``chunks`` = [(first, count), ...]: one block, or the two equal
        chunks of a folded frequency shard; T_rows [lmax+1, sum(count), F] in local channel order."""
        nnu = sum(int(c[1]) for c in chunks)
        assert tuple(T_rows.shape) == (lmax + 1, nnu, F), T_rows.shape
        alm = self._alm_out(lmax, nnu, out)
        cs = _chanset(chunks)
        _check(self.lib.corahip_draw_alm_philox_rows_set(self.h, self._f64(T_rows), self._p0(info),
                                                         c_u64(int(seed) & (2**64 - 1)), lmax, F, ctypes.byref(cs),
                                                         self._f64(alm)))
        return alm

    # -- frequency sharding: the data movements around the factor row-block all-to-all ---------
    def factor_rows_pack(self, T_local, l_stride, world):
        """[n_local, F, F] l-sharded factors -> send [world, l_stride, F / world, F] (slab q = rows of rank q's
        channels, l rows past n_local zero)."""
        n_local, F, _ = T_local.shape
        send = self.empty((world, l_stride, F // world, F))
        _check(self.lib.corahip_factor_rows_pack(self.h, self._f64(T_local) if n_local else None, n_local, l_stride, F,
                                                 world, self._f64(send)))
        return send

    def factor_rows_unpack(self, recv, counts):
        """recv [world, l_stride, nnu, F] (slab r from rank r) + the multipoles each rank holds -> T_rows
        [sum(counts), nnu, F], the l blocks in rank order."""
        world, l_stride, nnu, F = recv.shape
        cnt = (ctypes.c_int32 * world)(*[int(c) for c in counts])
        out = self.empty((int(sum(counts)), nnu, F))
        _check(self.lib.corahip_factor_rows_unpack(self.h, self._f64(recv), cnt, world, l_stride, nnu, F, self._f64(out)))
        return out

    def alm_dev_to_square(self, alm, lmax, nnu):
        torch = _torch()
        L = lmax + 1
        sq = torch.empty((nnu, 1, L, L), dtype=torch.complex128, device=self.device)
        _check(self.lib.corahip_alm_dev_to_square(self.h, self._f64(alm), lmax, nnu, self._p(sq)))
        return sq

    def alm_packed_to_dev(self, packed, lmax):
        torch = _torch()
        assert packed.dtype == torch.complex128
        nnu, nalm = packed.shape
        assert nalm == (lmax + 1) * (lmax + 2) // 2
        alm = self._alm_out(lmax, nnu)
        _check(self.lib.corahip_alm_packed_to_dev(self.h, self._p(packed), lmax, nnu, self._f64(alm)))
        return alm

    def alm_cross_spectra(self, alm_a, nx, lmax, alm_b=None, ny=None, out=None):
        """The multi-frequency spectrum of a_lm in the device layout, ``[lmax + 1, nx, ny]`` (clarray's layout):
        ``out[l, i, j] = sum_m c_m (Re a_i Re b_j + Im a_i Im b_j) / (2l + 1)``, ``c_0 = 1``, ``c_{m>0} = 2`` - healpy's
        ``alm2cl`` for every pair of channels, one FP64 MFMA Gram product per l (``corahip_alm_cross_spectra``).

        ``alm_a`` [nalm, ceil(nx / 4), 2, 4] as ``map2alm`` and ``draw_alm*`` return it; ``alm_b`` (with ``ny``) a second
        operand of the same lmax, ``None`` (or ``alm_a`` itself): the symmetric case, whose result equals its transpose
        bit for bit.  Padding channels never reach the result.  Two calls return identical bits."""
        nalm = (lmax + 1) * (lmax + 2) // 2
        nx = int(nx)
        if tuple(alm_a.shape) != (nalm, (nx + 3) // 4, 2, 4):
            raise ValueError("alm_a must be [nalm, ceil(nx / 4), 2, 4] (got %r)" % (tuple(alm_a.shape),))
        if alm_b is None:
            if ny is not None and int(ny) != nx:
                raise ValueError("ny goes with a second operand")
            ny = nx
        else:
            ny = nx if ny is None else int(ny)
            if tuple(alm_b.shape) != (nalm, (ny + 3) // 4, 2, 4):
                raise ValueError("alm_b must be [nalm, ceil(ny / 4), 2, 4] (got %r)" % (tuple(alm_b.shape),))
        if out is None:
            out = self.empty((lmax + 1, nx, ny))
        if tuple(out.shape) != (lmax + 1, nx, ny):
            raise ValueError("Given output array is incompatible.")
        _check(self.lib.corahip_alm_cross_spectra(self.h, self._f64(alm_a), nx, None if alm_b is None else self._f64(alm_b),
                                                  ny, int(lmax), self._f64(out)))
        return out

    def alm_gather_channels(self, src, nsrc, idx, dst, ndst, dst_first=0):
        """Channel ``dst_first + j`` of ``dst`` = channel ``idx[j]`` of ``src`` for every j, both a_lm buffers in the
        device layout ``[nalm, G, 2, 4]`` of the same lmax (``corahip_alm_gather_channels``): a streaming copy, bit for
        bit, that writes nothing of ``dst`` outside those channels - the other channels of a shared group and the
        padding keep what they held.  Returns ``dst``.

        ``src`` has ``ceil(nsrc / 4)`` groups and ``dst`` ``ceil(ndst / 4)``: a buffer padded to 8 channels (what
        ``map2alm_spin2`` returns) is passed with ``nsrc = 4 * src.shape[1]``.  ``idx``: a host sequence or a device
        tensor of int32 (host integer arrays of another width are converted), checked here on the host - one entry at
        least, every entry in ``[0, nsrc)``, ``dst_first + len(idx) <= ndst`` - ``ValueError`` otherwise; repeats are
        fine.  ``dst`` must not overlap ``src``."""
        torch = _torch()
        nsrc, ndst, dst_first = int(nsrc), int(ndst), int(dst_first)
        for t, name in ((src, "src"), (dst, "dst")):
            if (not isinstance(t, torch.Tensor) or t.dim() != 4 or tuple(t.shape[2:]) != (2, 4) or t.dtype != torch.float64
                    or t.device != self.device or not t.is_contiguous()):
                raise ValueError("%s must be a contiguous float64 [nalm, G, 2, 4] tensor on %s" % (name, self.device))
        nalm = int(src.shape[0])
        lmax = int(round((np.sqrt(8.0 * nalm + 1.0) - 3.0) / 2.0))
        if nalm < 1 or (lmax + 1) * (lmax + 2) // 2 != nalm or int(dst.shape[0]) != nalm:
            raise ValueError("src and dst must hold the (lmax + 1)(lmax + 2) / 2 coefficients of one lmax (got %d and %d rows)"
                             % (nalm, int(dst.shape[0])))
        if nsrc < 1 or int(src.shape[1]) != (nsrc + 3) // 4:
            raise ValueError("src has %d channel groups, nsrc = %d needs %d" % (int(src.shape[1]), nsrc, (nsrc + 3) // 4))
        if ndst < 1 or int(dst.shape[1]) != (ndst + 3) // 4:
            raise ValueError("dst has %d channel groups, ndst = %d needs %d" % (int(dst.shape[1]), ndst, (ndst + 3) // 4))
        if isinstance(idx, torch.Tensor):
            if idx.dtype != torch.int32:
                raise ValueError("idx must be int32 (got %s)" % idx.dtype)
            host = idx.detach().cpu().numpy()
        else:
            host = np.asarray(idx)
            if host.dtype.kind not in "iu":
                raise ValueError("idx must hold integers (got dtype %s)" % host.dtype)
        if host.ndim != 1 or host.size < 1:
            raise ValueError("idx must be one-dimensional with at least one entry (got shape %r)" % (host.shape,))
        n = int(host.size)
        if int(host.min()) < 0 or int(host.max()) >= nsrc:
            raise ValueError("idx must lie in [0, %d) (got %d .. %d)" % (nsrc, int(host.min()), int(host.max())))
        if dst_first < 0 or dst_first + n > ndst:
            raise ValueError("channels %d .. %d do not fit the %d channels of dst" % (dst_first, dst_first + n - 1, ndst))
        if self._overlap(dst, dst.numel() * 8, src, src.numel() * 8):
            raise ValueError("alm_gather_channels: dst overlaps src")
        if not (isinstance(idx, torch.Tensor) and idx.device == self.device and idx.is_contiguous()):
            idx = self.to_device(host, dtype=np.int32)
        _check(self.lib.corahip_alm_gather_channels(self.h, self._f64(src), nsrc, self._p(idx), n, lmax, self._f64(dst), ndst,
                                                    dst_first))
        return dst

    # -- K4/K5 ------------------------------------------------------------------------
    # truncation exponent of the Legendre sums used by plans made without an explicit one (0 = the library's
    # default, 2^-70); `Context.sht_cut_exp = -900` before the first transform keeps every representable term
    sht_cut_exp = 0

    def sht_plan(self, nside, lmax, cut_exp=None):
        """The (nside, lmax) transform plan; terms of the Legendre sums below 2^cut_exp are dropped (pixel error
        <= 2 sum |a_lm| 2^cut_exp; default -70, see corahip_sht_plan_create_ex)."""
        cut = int(self.sht_cut_exp if cut_exp is None else cut_exp)
        key = (int(nside), int(lmax)) if cut == 0 else (int(nside), int(lmax), cut)
        if key not in self._plans:
            h = c_void_p()
            _check(self.lib.corahip_sht_plan_create_ex(self.h, key[0], key[1], cut, ctypes.byref(h)))
            self._plans[key] = h
        return self._plans[key]

    def k4_mfma_count(self, nside, lmax, nnu, cut_exp=None):
        """FP64 MFMA instructions (v_mfma_f64_16x16x4_f64, 2048 flop each) the Legendre kernel issues for one
        alm2map pass over ``nnu`` channels - from the plan's tables, equal to the SQ_INSTS_VALU_MFMA_F64 counter."""
        n = c_u64()
        _check(self.lib.corahip_sht_plan_k4_mfma_count(self.h, self.sht_plan(nside, lmax, cut_exp), int(nnu), ctypes.byref(n)))
        return int(n.value)

    def alm2map_workspace_bytes(self, plan, nnu):
        b = c_size_t()
        _check(self.lib.corahip_alm2map_workspace_bytes(plan, nnu, ctypes.byref(b)))
        return int(b.value)

    def workspace(self, nbytes):
        torch = _torch()
        if self._workspace is None or self._workspace.numel() < nbytes:
            self._workspace = None
            self._workspace = torch.empty((nbytes,), dtype=torch.uint8, device=self.device)
        return self._workspace

    def alm2map(self, alm, nside, lmax, nnu, out=None, max_workspace_bytes=None, cut_exp=None):
        plan = self.sht_plan(nside, lmax, cut_exp)
        npix = 12 * nside * nside
        maps = out if out is not None else self.empty((nnu, npix))
        need = self.alm2map_workspace_bytes(plan, nnu)
        if max_workspace_bytes is not None:
            need = min(need, int(max_workspace_bytes))
        ws = self.workspace(need)
        _check(self.lib.corahip_alm2map(self.h, plan, self._f64(alm), nnu, self._f64(maps), self._p(ws), need))
        return maps

    def mkfullsky_fused(self, C, nside, rng, nu0=0, nnu=None, alms=False, workspace_bytes=None, workspace=None):
        """``corahip_mkfullsky``: C [L, F, F] (device) -> maps [nnu, npix] or, with ``alms``, a_lm [nnu, 1, L, L] complex,
        in one library call.  ``rng``: ("pcg64", state, inc) python ints of a numpy bit generator - returns the state
        after the draws -, ("stream", g) device normals in stream order, or ("philox", seed).  ``workspace``: a caller's
        uint8 device buffer of at least the bytes the call takes (default: a fresh one).  Returns (out, state)."""
        torch = _torch()
        L, F = int(C.shape[0]), int(C.shape[1])
        lmax = L - 1
        nnu = F if nnu is None else nnu
        plan = self.sht_plan(nside, lmax)

        kind = {"stream": 0, "philox": 1, "pcg64": 2, "legacy": 3}[rng[0]]
        if kind >= 2:        # ("legacy", np.random.get_state(legacy=False)): returns the state dict after the draws
            r, ms = _rng_struct(rng)
        else:
            r, ms = _Rng(), None
            r.kind = kind
            if kind == 0:
                r.stream = self._f64(rng[1])
            else:
                r.seed = int(rng[1]) & (2**64 - 1)
        b = c_size_t()
        _check(self.lib.corahip_mkfullsky_workspace_bytes(plan, F, nu0, nnu, kind, 1 if alms else 0, ctypes.byref(b)))
        need = int(b.value) if workspace_bytes is None else int(workspace_bytes)
        if workspace is None:
            ws = torch.empty((max(need, 1),), dtype=torch.uint8, device=self.device)
        else:
            ws = workspace
            assert ws.dtype == torch.uint8 and ws.device == self.device and ws.numel() >= need, (ws.numel(), need)
        out = (torch.empty((nnu, 1, L, L), dtype=torch.complex128, device=self.device) if alms
               else self.empty((nnu, 12 * nside * nside)))
        _check(self.lib.corahip_mkfullsky(self.h, plan, self._f64(C), F, ctypes.byref(r), nu0, nnu, 1 if alms else 0,
                                          c_void_p(out.data_ptr()), self._p(ws), need))
        if kind == 3:
            return out, _mt_dict(ms)
        return out, ((int(r.state[0]) << 64) | int(r.state[1])) if kind == 2 else None

    def map2alm_workspace_bytes(self, plan, nnu):
        b = c_size_t()
        _check(self.lib.corahip_map2alm_workspace_bytes(plan, nnu, ctypes.byref(b)))
        return int(b.value)

    def map2alm(self, maps, nside, lmax, ring_w=None, chunk=None, out=None):
        """One weighted quadrature pass maps [nnu, npix] -> alm_dev [nalm, ceil(nnu/4), 2, 4] (K5^T + K4^T).

        ring_w: device [2 nside] north-ring weights or None.  Channels go through in chunks of `chunk`
        (a multiple of 8; default: as many as a 96 GB workspace holds).  out: the alm_dev buffer to write."""
        torch = _torch()
        plan = self.sht_plan(nside, lmax)
        nnu, npix = maps.shape
        assert npix == 12 * nside * nside
        nalm = (lmax + 1) * (lmax + 2) // 2
        G4 = (nnu + 3) // 4
        if chunk is None:
            per8 = self.map2alm_workspace_bytes(plan, 8)
            chunk = max(8, min((int(96e9 // per8)) * 8, (nnu + 7) // 8 * 8))
        assert chunk % 8 == 0
        if out is None:
            out = self.empty((nalm, G4, 2, 4))
        assert tuple(out.shape) == (nalm, G4, 2, 4), out.shape
        for c0 in range(0, nnu, chunk):
            n = min(chunk, nnu - c0)
            G8 = (n + 7) // 8 * 2
            need = self.map2alm_workspace_bytes(plan, n)
            ws = self.workspace(need)
            part = out if (c0 == 0 and n == nnu and G8 == G4) else self.empty((nalm, G8, 2, 4))
            _check(self.lib.corahip_map2alm(self.h, plan, self._f64(maps[c0:c0 + n]), n,
                                            self._f64(ring_w) if ring_w is not None else None, self._f64(part),
                                            self._p(ws), need))
            if part is not out:
                g0 = c0 // 4
                gn = min(G8, G4 - g0)
                out[:, g0:g0 + gn].copy_(part[:, :gn])
        return out

    def alm2map_spin2(self, alm, nside, lmax, nnu, out=None):
        """alm_dev of nnu = 2 nfreq interleaved (E, B) channels -> maps [nnu, npix] = interleaved (Q, U)."""
        plan = self.sht_plan(nside, lmax)
        maps = out if out is not None else self.empty((nnu, 12 * nside * nside))
        need = self.alm2map_workspace_bytes(plan, nnu)
        ws = self.workspace(need)
        _check(self.lib.corahip_alm2map_spin2(self.h, plan, self._f64(alm), nnu, self._f64(maps), self._p(ws), need))
        return maps

    # -- spin-2 analysis (composition of scalar passes) ---------------------------------------
    def map2alm_spin2(self, maps_qu, nside, lmax, ring_w=None, out=None):
        """One quadrature pass (Q_f, U_f interleaved) [2 nf, npix] -> alm_dev [nalm, G, 2, 4] with (E_f, B_f)
        interleaved, G = nnu_pad8(2 nf) / 4 (the layout alm2map_spin2 takes); out: the alm_dev buffer to write."""
        plan = self.sht_plan(nside, lmax)
        n2, npix = maps_qu.shape
        assert n2 % 2 == 0 and npix == 12 * nside * nside
        nf = n2 // 2
        nalm = (lmax + 1) * (lmax + 2) // 2
        maps6 = self.empty((6 * nf, npix))
        _check(self.lib.corahip_spin2_ring_scale(self.h, plan, self._f64(maps_qu), nf, self._f64(maps6)))
        a6 = self.map2alm(maps6, nside, lmax, ring_w)
        del maps6
        gout = (2 * nf + 7) // 8 * 2
        if out is None:
            out = self.empty((nalm, gout, 2, 4))
        assert tuple(out.shape) == (nalm, gout, 2, 4), out.shape
        _check(self.lib.corahip_spin2_combine(self.h, plan, self._f64(a6), a6.shape[1], nf, self._f64(out), gout))
        return out

    # -- spin-2 analysis (one Legendre pass, csrc/sht_polana_native.hip) ----------------------
    def map2alm_spin2_workspace_bytes(self, plan, nfields):
        b = c_size_t()
        _check(self.lib.corahip_map2alm_spin2_workspace_bytes(plan, nfields, ctypes.byref(b)))
        return int(b.value)

    def map2alm_spin2_native(self, maps_qu, nside, lmax, ring_w=None, chunk=None, out=None):
        """The quadrature pass of ``map2alm_spin2`` as one Legendre pass (K5^T on the 2 nf channels + the adjoint of the
        spin-2 synthesis kernel): same arguments, same layout of the result, no scaled copies of the maps.

        Fields go through in chunks of `chunk` (a multiple of 4, so that every chunk fills whole 8-channel groups;
        default: as many as a 96 GB workspace holds)."""
        plan = self.sht_plan(nside, lmax)
        n2, npix = maps_qu.shape
        assert n2 % 2 == 0 and npix == 12 * nside * nside
        nf = n2 // 2
        nalm = (lmax + 1) * (lmax + 2) // 2
        gout = (2 * nf + 7) // 8 * 2
        if chunk is None:
            per4 = self.map2alm_spin2_workspace_bytes(plan, 4)
            chunk = max(4, min((int(96e9 // per4)) * 4, (nf + 3) // 4 * 4))
        assert chunk >= 4 and chunk % 4 == 0
        if out is None:
            out = self.empty((nalm, gout, 2, 4))
        assert tuple(out.shape) == (nalm, gout, 2, 4), out.shape
        w = self._f64(ring_w) if ring_w is not None else None
        for f0 in range(0, nf, chunk):
            n = min(chunk, nf - f0)
            gn = (2 * n + 7) // 8 * 2
            need = self.map2alm_spin2_workspace_bytes(plan, n)
            ws = self.workspace(need)
            part = out if (f0 == 0 and n == nf) else self.empty((nalm, gn, 2, 4))
            _check(self.lib.corahip_map2alm_spin2(self.h, plan, self._f64(maps_qu[2 * f0:2 * (f0 + n)]), n, w,
                                                  self._f64(part), self._p(ws), need))
            if part is not out:
                out[:, f0 // 2:f0 // 2 + gn].copy_(part)
        return out

    # -- derivative synthesis (composition around the scalar synthesis, csrc/sht_der1.hip) --------------
    def der1_alm_prep(self, alm, nside, lmax, g0=0, g_in=None, out=None):
        """Channel groups g0 .. g0 + g_in - 1 of alm_dev [nalm, G, 2, 4] -> alm3_dev [nalm, 3 g_in, 2, 4], group blocks
        [l a | c_{l+1,m} a_{l+1,m} | i m a] (corahip_der1_alm_prep)."""
        plan = self.sht_plan(nside, lmax)
        nalm = (lmax + 1) * (lmax + 2) // 2
        G = int(alm.shape[1])
        g_in = G - g0 if g_in is None else int(g_in)
        assert tuple(alm.shape) == (nalm, G, 2, 4), alm.shape
        a3 = out if out is not None else self.empty((nalm, 3 * g_in, 2, 4))
        assert tuple(a3.shape) == (nalm, 3 * g_in, 2, 4), a3.shape
        _check(self.lib.corahip_der1_alm_prep(self.h, plan, self._f64(alm), G, int(g0), g_in, self._f64(a3)))
        return a3

    def der1_combine(self, maps3, nside, lmax, g_in, nfields, out_theta, out_phi, scale_theta=None, scale_phi=None,
                     phi_extra=0):
        """maps3 [12 g_in, npix] (the synthesis of alm3_dev) -> out_theta, out_phi [nfields, npix]
        (corahip_der1_combine); scale_theta / scale_phi: device [nfields] per-field factors or None."""
        plan = self.sht_plan(nside, lmax)
        npix = 12 * nside * nside
        assert tuple(maps3.shape) == (12 * g_in, npix), maps3.shape
        assert tuple(out_theta.shape) == (nfields, npix) and tuple(out_phi.shape) == (nfields, npix)
        for s in (scale_theta, scale_phi):
            assert s is None or s.numel() == nfields
        _check(self.lib.corahip_der1_combine(self.h, plan, self._f64(maps3), int(g_in), int(nfields),
                                             None if scale_theta is None else self._f64(scale_theta),
                                             None if scale_phi is None else self._f64(scale_phi), int(phi_extra),
                                             self._f64(out_theta), self._f64(out_phi)))
        return out_theta, out_phi

    def alm2map_der1_bytes(self, nside, lmax, nfields=16):
        """Device bytes :meth:`alm2map_der1` takes for a chunk of ``nfields`` fields: alm3 (3 coefficient sets) + the
        three synthesised maps per field + the synthesis workspace of 3 x 4 ceil(nfields / 4) channels."""
        g = (int(nfields) + 3) // 4
        nalm = (lmax + 1) * (lmax + 2) // 2
        ws = self.alm2map_workspace_bytes(self.sht_plan(nside, lmax), 12 * g)
        return nalm * 3 * g * 64 + 12 * g * 12 * nside * nside * 8 + ws

    def alm2map_der1(self, alm, nside, lmax, nnu, scale_theta=None, scale_phi=None, phi_extra=0, out=None,
                     max_bytes=None):
        """healpy.alm2map_der1 without its first row: alm_dev [nalm, G, 2, 4] of ``nnu`` fields ->
        ``(dT/dtheta, (1/sin theta) dT/dphi)``, two device tensors [nnu, npix] (``out``: the pair to write, e.g. two
        rows of a displacement field).  T itself is :meth:`alm2map`.

        ``scale_theta`` / ``scale_phi``: device [nnu] factors multiplied into the components of each field;
        ``phi_extra=1`` divides the phi component by sin theta once more.  Both are applied by the combining kernel.

        The fields go through prep -> alm2map over 3 x 4 channels per group of four fields -> combine in chunks of
        whole groups whose temporaries (:meth:`alm2map_der1_bytes`) stay within ``max_bytes``; default: what 16 fields
        need at this nside and lmax (12.9e9 bytes at nside 1024, lmax 2048).  A chunk is never smaller than one
        group.  The result does not depend on the chunking beyond the rounding of the synthesis."""
        npix = 12 * nside * nside
        G = int(alm.shape[1])
        assert 1 <= nnu <= 4 * G
        if out is None:
            out = (self.empty((nnu, npix)), self.empty((nnu, npix)))
        ot, op = out
        assert tuple(ot.shape) == (nnu, npix) and tuple(op.shape) == (nnu, npix)
        budget = self.alm2map_der1_bytes(nside, lmax, 16) if max_bytes is None else int(max_bytes)
        gall = (nnu + 3) // 4
        gc = gall
        while gc > 1 and self.alm2map_der1_bytes(nside, lmax, 4 * gc) > budget:
            gc -= 1
        plan = self.sht_plan(nside, lmax)
        for g0 in range(0, gall, gc):
            g = min(gc, gall - g0)
            f0, nf = 4 * g0, min(4 * g, nnu - 4 * g0)
            a3 = self.der1_alm_prep(alm, nside, lmax, g0, g)
            maps3 = self.empty((12 * g, npix))
            need = self.alm2map_workspace_bytes(plan, 12 * g)
            ws = self.workspace(need)
            _check(self.lib.corahip_alm2map(self.h, plan, self._f64(a3), 12 * g, self._f64(maps3), self._p(ws), need))
            del a3
            self.der1_combine(maps3, nside, lmax, g, nf, ot[f0:f0 + nf], op[f0:f0 + nf],
                              None if scale_theta is None else scale_theta[f0:f0 + nf],
                              None if scale_phi is None else scale_phi[f0:f0 + nf], phi_extra)
            del maps3
        return ot, op

    @staticmethod
    def gradient_coefficients(x):
        """Host table [n, 3] of numpy.gradient's coefficients (a, b, c) for coordinates ``x`` (edge_order 1):
        interior ``a = -hd / (hs (hd + hs))``, ``b = (hd - hs) / (hd hs)``, ``c = hs / (hd (hd + hs))`` with
        ``hd = x[i+1] - x[i]``, ``hs = x[i] - x[i-1]``; first row (0, -1/h, 1/h), last row (-1/h, 1/h, 0)."""
        x = np.asarray(x, dtype=np.float64)
        n = x.size
        if x.ndim != 1 or n < 2:
            raise ValueError("gradient needs at least 2 coordinates along the axis (got shape %r)" % (x.shape,))
        d = np.diff(x)
        coef = np.zeros((n, 3))
        hs, hd = d[:-1], d[1:]
        coef[1:-1, 0] = -hd / (hs * (hd + hs))
        coef[1:-1, 1] = (hd - hs) / (hd * hs)
        coef[1:-1, 2] = hs / (hd * (hd + hs))
        coef[0, 1], coef[0, 2] = -1.0 / d[0], 1.0 / d[0]
        coef[-1, 0], coef[-1, 1] = -1.0 / d[-1], 1.0 / d[-1]
        return coef

    def radial_gradient(self, f, x, scale=None, out=None):
        """``numpy.gradient(f, x, axis=0) * scale[:, None]`` of a device array f [n, npix] (n >= 2) for host
        coordinates ``x`` [n] (any spacing, ascending or descending); ``scale``: host or device [n] or None.
        ``out`` must not share memory with ``f`` (ValueError)."""
        torch = _torch()
        if f.dim() != 2:
            raise ValueError("radial_gradient takes a [n, npix] array (got %r)" % (tuple(f.shape),))
        n, npix = f.shape
        coef = self.gradient_coefficients(x)
        if coef.shape[0] != n:
            raise ValueError("x has %d entries, f %d rows" % (coef.shape[0], n))
        if out is None:
            out = self.empty((n, npix))
        if tuple(out.shape) != (n, npix):
            raise ValueError("out has shape %r, expected %r" % (tuple(out.shape), (n, npix)))
        nbytes = n * npix * 8
        if out.data_ptr() < f.data_ptr() + nbytes and f.data_ptr() < out.data_ptr() + nbytes:
            raise ValueError("radial_gradient: out overlaps f")
        if scale is not None and not isinstance(scale, torch.Tensor):
            scale = self.to_device(np.asarray(scale, dtype=np.float64))
        if scale is not None and scale.numel() != n:
            raise ValueError("scale has %d entries, f %d rows" % (scale.numel(), n))
        cdev = self.to_device(coef)
        _check(self.lib.corahip_radial_gradient(self.h, self._f64(f), self._f64(cdev),
                                                None if scale is None else self._f64(scale), int(n), int(npix),
                                                self._f64(out)))
        return out

    # -- LSS chain: bias, linear dynamics, Fingers of God, map (csrc/lsschain.hip) -----------------------------------
    def _rowvec(self, v, n, name):
        """``[n]`` host array, scalar (broadcast) or device tensor -> device float64 [n]."""
        torch = _torch()
        if isinstance(v, torch.Tensor):
            v = v.to(device=self.device, dtype=torch.float64).reshape(-1)
            if v.numel() == 1:
                v = v.expand(n)
            v = v.contiguous()
        else:
            h = np.asarray(v, dtype=np.float64)
            if h.ndim == 0:
                h = np.full(n, float(h))
            v = self.to_device(h.reshape(-1))
        if v.numel() != n:
            raise ValueError("Array %s has %d entries, expected %d" % (name, v.numel(), n))
        return v

    def _field2d(self, f, name):
        torch = _torch()
        if not isinstance(f, torch.Tensor) or f.dim() != 2:
            raise ValueError("%s must be a [n, ncol] device tensor (got shape %r)" % (name, tuple(getattr(f, "shape", ()))))
        if f.dtype != torch.float64 or not f.is_contiguous():
            raise ValueError("%s must be a contiguous float64 tensor" % name)
        return int(f.shape[0]), int(f.shape[1])

    @staticmethod
    def _overlap(a, abytes, b, bbytes):
        return a.data_ptr() < b.data_ptr() + bbytes and b.data_ptr() < a.data_ptr() + abytes

    @staticmethod
    def slice_mix_ranges(K, band_cut=None):
        """Host side of the skipping rule of ``slice_mix``: ``(K', ranges)`` for a host matrix ``K`` [n, n].

        With ``band_cut`` the entries with ``|K_ij| < band_cut * max_j |K_ij|`` are zeroed in the copy ``K'`` (else
        ``K'`` is ``K``).  ``ranges`` is int32 [ceil(n / 16), 2]: for each block of 16 output rows the range
        ``[klo, khi)`` of input slices that holds every non-zero entry of those rows of ``K'``, widened to multiples
        of the MFMA depth 4 (``khi`` may exceed n by up to 3: the kernel pads with zeros); (0, 0) for an all-zero
        block."""
        K = np.asarray(K, dtype=np.float64)
        if K.ndim != 2 or K.shape[0] != K.shape[1]:
            raise ValueError("K must be a square matrix (got shape %r)" % (K.shape,))
        n = K.shape[0]
        if band_cut is not None:
            K = np.where(np.abs(K) < float(band_cut) * np.abs(K).max(axis=1, keepdims=True), 0.0, K)
        nb = (n + 15) // 16
        ranges = np.zeros((nb, 2), dtype=np.int32)
        for b in range(nb):
            cols = np.nonzero((K[16 * b:16 * b + 16] != 0).any(axis=0))[0]
            if cols.size:
                ranges[b] = (cols[0] // 4 * 4, (cols[-1] + 4) // 4 * 4)
        return K, ranges

    def slice_mix(self, K, f, out=None, band_cut=None, skip=True, ranges=None):
        """``out = K @ f`` for a device field ``f`` [n, ncol] and a matrix ``K`` [n, n] (host array or device tensor),
        1 <= n <= 4096, with FP64 MFMA.  ``out`` must not overlap ``f`` (ValueError).

        The host passes, per block of 16 output rows, the range of input slices outside which the rows of ``K`` are
        exactly zero (:meth:`slice_mix_ranges`); the kernel forms no product outside it.  Those terms are exact zeros:
        for finite ``f`` the result does not depend on the skipping (``skip=False`` passes no ranges and gives the
        same bits).  A non-finite ``f`` in a skipped slice does not propagate, where a dense product gives NaN.

        ``band_cut``: entries with ``|K_ij| < band_cut * max_j |K_ij|`` are zeroed in a copy of ``K`` first, which
        narrows the ranges of a banded kernel.  What that drops from element (i, p) is bounded by
        ``band_cut * max_j |K_ij| * sum_j |f_jp|``.  Default ``None``: exact, like the reference's ``np.matmul``.
        Two calls on the same inputs return identical bits (no atomics).

        ``ranges``: a device int32 tensor from an earlier ``to_device(slice_mix_ranges(K)[1], np.int32)`` for the same
        device matrix ``K``: the call then does no host work on ``K`` (repeated products with one matrix)."""
        torch = _torch()
        n, ncol = self._field2d(f, "f")
        if ranges is not None:
            if not isinstance(K, torch.Tensor) or band_cut is not None or tuple(K.shape) != (n, n):
                raise ValueError("slice_mix: ranges go with a device matrix K [n, n] and no band_cut")
            if ranges.dtype != torch.int32 or tuple(ranges.shape) != ((n + 15) // 16, 2) or not ranges.is_contiguous():
                raise ValueError("slice_mix: ranges must be int32 [ceil(n / 16), 2]")
            return self._slice_mix_launch(K, f, out, ranges, n, ncol)
        Kh = K.detach().cpu().numpy() if isinstance(K, torch.Tensor) else np.asarray(K, dtype=np.float64)
        if Kh.shape != (n, n):
            raise ValueError("Array K has the wrong shape (got %r, expected %r)" % (tuple(Kh.shape), (n, n)))
        if not 1 <= n <= 4096:
            raise ValueError("slice_mix takes 1 <= n <= 4096 slices (got %d)" % n)
        Kc, ranges = self.slice_mix_ranges(Kh, band_cut)
        if isinstance(K, torch.Tensor) and band_cut is None and K.dtype == torch.float64 and K.is_contiguous() \
                and K.device == self.device:
            Kd = K
        else:
            Kd = self.to_device(Kc)
        rdev = self.to_device(ranges, dtype=np.int32) if skip else None
        return self._slice_mix_launch(Kd, f, out, rdev, n, ncol)

    def _slice_mix_launch(self, Kd, f, out, rdev, n, ncol):
        torch = _torch()
        if out is None:
            out = self.empty((n, ncol))
        if tuple(out.shape) != (n, ncol) or out.dtype != torch.float64 or not out.is_contiguous():
            raise ValueError("out must be a contiguous float64 [%d, %d] tensor" % (n, ncol))
        if self._overlap(out, n * ncol * 8, f, n * ncol * 8) or self._overlap(out, n * ncol * 8, Kd, n * n * 8):
            raise ValueError("slice_mix: out overlaps an input")
        _check(self.lib.corahip_slice_mix(self.h, self._f64(Kd), self._f64(f), None if rdev is None else self._p(rdev),
                                          n, ncol, self._f64(out)))
        return out

    @staticmethod
    def diff2_coefficients(x):
        """Host tables of ``lssutil.diff2`` (cora/signal/lssutil.py:99-185) for coordinates ``x`` [n], n >= 4:
        ``(coef [n, 4], first [n])``.  Output row i is ``((c0 w0 + c1 w1) + c2 w2) + c3 w3`` over the input rows
        ``first[i] .. first[i] + 3`` (``first[i] = min(max(i - 2, 0), n - 4)``, the rule the kernel applies).  Interior
        rows 2 .. n - 2 hold ``(alpha, beta, -(alpha + beta + gamma), gamma)`` of the reference, rows 0, 1 and n - 1 its
        one-sided 4-point weights, each from the reference's expression."""
        x = np.asarray(x, dtype=np.float64)
        n = x.size
        if x.ndim != 1 or n < 4:
            raise ValueError("diff2 needs at least 4 coordinates along the axis (got shape %r)" % (x.shape,))
        coef = np.zeros((n, 4))
        for i in range(2, n - 1):
            dm2 = x[i] - x[i - 2]
            dm1 = x[i] - x[i - 1]
            dp1 = x[i + 1] - x[i]
            alpha = 2 * (dp1 - dm1) / (dm2 * (dm2 + dp1) * (dm2 - dm1))
            beta = 2 * (dm2 - dp1) / (dm1 * (dm2 - dm1) * (dm1 + dp1))
            gamma = 2 * (dm2 + dm1) / (dp1 * (dm1 + dp1) * (dm2 + dp1))
            coef[i] = (alpha, beta, -(alpha + beta + gamma), gamma)
        dp1, dp2, dp3 = x[1] - x[0], x[2] - x[0], x[3] - x[0]
        coef[0] = (2 * (dp1 + dp2 + dp3) / (dp1 * dp2 * dp3),
                   -2 * (dp2 + dp3) / (dp1 * (dp1 - dp2) * (dp1 - dp3)),
                   2 * (dp1 + dp3) / ((dp1 - dp2) * dp2 * (dp2 - dp3)),
                   2 * (dp1 + dp2) / ((dp1 - dp3) * dp3 * (-dp2 + dp3)))
        dm1, dp1, dp2 = x[1] - x[0], x[2] - x[1], x[3] - x[1]
        coef[1] = (2 * (dp1 + dp2) / (dm1 * (dm1 + dp1) * (dm1 + dp2)),
                   2 * (dm1 - dp1 - dp2) / (dm1 * dp1 * dp2),
                   2 * (dm1 - dp2) / (dp1 * (dm1 + dp1) * (dp1 - dp2)),
                   -2 * (dm1 - dp1) / ((dp1 - dp2) * dp2 * (dm1 + dp2)))
        dm1, dm2, dm3 = x[-1] - x[-2], x[-1] - x[-3], x[-1] - x[-4]
        coef[n - 1] = (2 * (dm1 + dm2) / ((dm1 - dm3) * dm3 * (-dm2 + dm3)),
                       2 * (dm1 + dm3) / ((dm1 - dm2) * dm2 * (dm2 - dm3)),
                       -2 * (dm2 + dm3) / (dm1 * (dm1 - dm2) * (dm1 - dm3)),
                       2 * (dm1 + dm2 + dm3) / (dm1 * dm2 * dm3))
        first = np.clip(np.arange(n) - 2, 0, n - 4)
        return coef, first

    def slice_diff2(self, f, x, g=None, h=None, s=None, t=None, out=None, coef=None):
        """``lssutil.diff2(f, x, axis=0)`` of a device field f [n, ncol], n >= 4, equal to the reference bit for bit
        (the reference's operation order, no contraction).  With ``g``, ``h`` [n, ncol] and per-row factors ``s``,
        ``t``: ``out = (h + s[:, None] * g) + d2 * t[:, None]`` in one pass.  ``f=None`` (``x`` unused): ``out = h +
        s[:, None] * g``.  ``out`` must not overlap ``f``; it may be ``g`` or ``h`` (an element is read before it is
        written, by the same thread).

        ``coef``: a ready-made host table [n, 4] in place of ``diff2_coefficients(x)`` (``x`` is then unused): any
        stencil over the same four rows ``first[i] .. first[i] + 3``, evaluated as ``((c0 w0 + c1 w1) + c2 w2) + c3 w3``
        (``lssutil.laplacian_device`` merges the radial terms of the Laplacian into one)."""
        if (g is None) != (h is None):
            raise ValueError("slice_diff2: g and h come together")
        ref = f if f is not None else g
        if ref is None:
            raise ValueError("slice_diff2 needs f or (g, h)")
        n, ncol = self._field2d(ref, "f" if f is not None else "g")
        cdev = None
        if f is not None:
            if coef is None:
                coef, _ = self.diff2_coefficients(x)
                if coef.shape[0] != n:
                    raise ValueError("x has %d entries, f %d rows" % (coef.shape[0], n))
            else:
                coef = np.asarray(coef, dtype=np.float64)
                if coef.shape != (n, 4) or n < 4:
                    raise ValueError("coef has shape %r, expected %r with at least 4 rows" % (coef.shape, (n, 4)))
            cdev = self.to_device(coef)
        for a, name in ((g, "g"), (h, "h")):
            if a is not None and self._field2d(a, name) != (n, ncol):
                raise ValueError("Array %s has the wrong shape (got %r, expected %r)" % (name, tuple(a.shape), (n, ncol)))
        sd = td = None
        if g is not None:
            sd = self._rowvec(s, n, "s")
            td = self._rowvec(t, n, "t") if f is not None else None
        if out is None:
            out = self.empty((n, ncol))
        if self._field2d(out, "out") != (n, ncol):
            raise ValueError("out has shape %r, expected %r" % (tuple(out.shape), (n, ncol)))
        if f is not None and self._overlap(out, n * ncol * 8, f, n * ncol * 8):
            raise ValueError("slice_diff2: out overlaps f")
        opt = lambda a: None if a is None else self._f64(a)  # noqa: E731
        _check(self.lib.corahip_slice_diff2(self.h, opt(f), opt(cdev), opt(g), opt(h), opt(sd), opt(td), n, ncol,
                                            self._f64(out)))
        return out

    def slice_moments(self, f, c=None):
        """``(sum_p (f[i, p] - c[i]), sum_p (f[i, p] - c[i])**2)`` per row of a device field f [n, ncol]; ``f`` may be a
        view with a row stride larger than ncol (unit column stride), ``c`` device [n] or None (= 0).  Fixed summation
        order: identical bits from call to call."""
        torch = _torch()
        if not isinstance(f, torch.Tensor) or f.dim() != 2 or f.dtype != torch.float64 or f.device != self.device:
            raise ValueError("slice_moments takes a float64 [n, ncol] device tensor")
        n, ncol = int(f.shape[0]), int(f.shape[1])
        ld = int(f.stride(0)) if n > 1 else ncol
        if n < 1 or ncol < 1 or (ncol > 1 and f.stride(1) != 1) or ld < ncol:
            raise ValueError("slice_moments: rows must be contiguous, row stride >= ncol")
        if c is not None:
            c = self._rowvec(c, n, "c")
        nbytes = c_size_t()
        _check(self.lib.corahip_slice_moments_workspace_bytes(n, ncol, ctypes.byref(nbytes)))
        work = torch.empty(int(nbytes.value) // 8, dtype=torch.float64, device=self.device)
        sums = self.empty((2, n))
        _check(self.lib.corahip_slice_moments(self.h, c_void_p(f.data_ptr()), ld, None if c is None else self._f64(c), n,
                                              ncol, self._p(work), int(nbytes.value), self._f64(sums[0]),
                                              self._f64(sums[1])))
        return sums[0], sums[1]

    def bias_field(self, delta, c1, c2=None, m2=None, out=None):
        """``out = c1[:, None] * delta + c2[:, None] * (delta**2 - m2[:, None])`` (``c2 is None``: exactly ``c1[:, None] *
        delta``) for a device field [n, ncol]; ``out`` may be ``delta`` itself."""
        n, ncol = self._field2d(delta, "delta")
        if (c2 is None) != (m2 is None):
            raise ValueError("bias_field: c2 and m2 come together")
        c1 = self._rowvec(c1, n, "c1")
        if c2 is not None:
            c2, m2 = self._rowvec(c2, n, "c2"), self._rowvec(m2, n, "m2")
        if out is None:
            out = self.empty((n, ncol))
        if self._field2d(out, "out") != (n, ncol):
            raise ValueError("out has shape %r, expected %r" % (tuple(out.shape), (n, ncol)))
        if out.data_ptr() != delta.data_ptr() and self._overlap(out, n * ncol * 8, delta, n * ncol * 8):
            raise ValueError("bias_field: out partly overlaps delta")
        _check(self.lib.corahip_bias_field(self.h, self._f64(delta), self._f64(c1), None if c2 is None else self._f64(c2),
                                           None if m2 is None else self._f64(m2), n, ncol, self._f64(out)))
        return out

    def lognormal(self, f, half_var, out=None, prefactor=1.0, row_scale=None):
        """``out = ((exp(f - half_var[:, None]) - 1) * prefactor) * row_scale[:, None]`` for a device field f [n, ncol];
        ``half_var=None``: no transform (``out = (f * prefactor) * row_scale``).  ``out`` [n, ncol] may be ``f`` itself
        or a view with a larger row stride, e.g. plane 0 ``m[:, 0]`` of a map ``m`` [n, 4, ncol]."""
        torch = _torch()
        n, ncol = self._field2d(f, "f")
        hv = None if half_var is None else self._rowvec(half_var, n, "half_var")
        rs = None if row_scale is None else self._rowvec(row_scale, n, "row_scale")
        if out is None:
            out = self.empty((n, ncol))
        if not isinstance(out, torch.Tensor) or tuple(out.shape) != (n, ncol) or out.dtype != torch.float64 \
                or out.device != self.device:
            raise ValueError("Given output array is incompatible.")
        ld = int(out.stride(0)) if n > 1 else ncol
        if (ncol > 1 and out.stride(1) != 1) or ld < ncol:
            raise ValueError("Given output array is incompatible.")
        inplace = out.data_ptr() == f.data_ptr() and ld == ncol
        if not inplace and self._overlap(out, ((n - 1) * ld + ncol) * 8, f, n * ncol * 8):
            raise ValueError("lognormal: out partly overlaps f")
        _check(self.lib.corahip_lognormal(self.h, self._f64(f), None if hv is None else self._f64(hv),
                                          None if rs is None else self._f64(rs), float(prefactor), n, ncol, ld,
                                          c_void_p(out.data_ptr())))
        return out

    # -- n3: xi(r) -> C_l --------------------------------------------------------------
    def xi_table_max_knots(self):
        """Largest spline table ``xi_table_average`` takes: it has to fit the LDS of one workgroup."""
        n = c_int(0)
        _check(self.lib.corahip_xi_table_max_knots(self.h, ctypes.byref(n)))
        return int(n.value)

    def xi_table_average(self, kx, ky, ky2, kind, x_t, f_t, mu, xa, xw, F, xint, out=None):
        nm = mu.numel()
        if out is None:
            out = self.empty((nm, F, F))
        if tuple(out.shape) != (nm, F, F) or not out.is_contiguous():
            raise ValueError("Given output array is incompatible.")
        _check(self.lib.corahip_xi_table_average(self.h, self._f64(kx), self._f64(ky), self._f64(ky2), kx.numel(), kind,
                                                 float(x_t), float(f_t), self._f64(mu), nm, self._f64(xa), self._f64(xw),
                                                 F, xint, self._f64(out)))
        return out

    def legendre_project(self, mu, wt, lmax, xi, out=None):
        nm = mu.numel()
        ncol = xi.numel() // nm
        if out is None:
            out = self.empty((lmax + 1, ncol))
        if tuple(out.shape) != (lmax + 1, ncol) or not out.is_contiguous():
            raise ValueError("Given output array is incompatible.")
        _check(self.lib.corahip_legendre_project(self.h, self._f64(mu), self._f64(wt), nm, lmax, self._f64(xi),
                                                 ncol, self._f64(out)))
        return out

    XI_MULTI_MAX = 4             # tables one ``xi_multi_average`` call takes

    def xi_multi_average(self, kx, ky, ky2, kind, x_t, f_t, mu, xa, xw, F, xint, nm_rows=None, out=None):
        """``corahip_xi_multi_average``: ``ky``, ``ky2`` [nfun, nk] on the knots ``kx`` [nk], ``f_t`` a host sequence
        [nfun] -> packed ``out`` [nm_rows, nfun, F (F + 1) / 2] (rows from ``mu.numel()`` on are zeros)."""
        nm, nk = mu.numel(), kx.numel()
        if ky.dim() != 2 or ky.shape[1] != nk or tuple(ky2.shape) != tuple(ky.shape):
            raise ValueError("xi_multi_average: ky and ky2 must be [nfun, %d] (got %s, %s)" % (nk, tuple(ky.shape), tuple(ky2.shape)))
        if not (kx.is_contiguous() and ky.is_contiguous() and ky2.is_contiguous()):
            raise ValueError("xi_multi_average: kx, ky and ky2 must be contiguous")
        nfun = int(ky.shape[0])
        f_t = np.ascontiguousarray(f_t, dtype=np.float64).reshape(-1)
        if f_t.size != nfun:
            raise ValueError("xi_multi_average: %d values of f_t for %d tables" % (f_t.size, nfun))
        nm_rows = nm if nm_rows is None else int(nm_rows)
        npair = F * (F + 1) // 2
        if out is None:
            out = self.empty((max(nm_rows, 0), nfun, npair))
        if tuple(out.shape) != (nm_rows, nfun, npair) or not out.is_contiguous():
            raise ValueError("Given output array is incompatible.")
        _check(self.lib.corahip_xi_multi_average(self.h, self._f64(kx), self._f64(ky), self._f64(ky2), nk, nfun, kind,
                                                 float(x_t), f_t.ctypes.data_as(ctypes.POINTER(c_double)), self._f64(mu),
                                                 nm, self._f64(xa), self._f64(xw), F, xint, nm_rows, self._f64(out)))
        return out

    def cl_blocks(self, packed, F, out=None):
        """``corahip_cl_blocks``: packed [L, npair] -> [L, F, F], or packed [L, 3, npair] (delta delta, phi delta, phi phi)
        -> the extended blocks [L, 2F, 2F] of the initial-LSS draw."""
        npair = F * (F + 1) // 2
        if packed.dim() not in (2, 3) or packed.shape[-1] != npair:
            raise ValueError("cl_blocks: packed must be [L, %d] or [L, nfun, %d] (got %s)" % (npair, npair, tuple(packed.shape)))
        if not packed.is_contiguous():
            raise ValueError("cl_blocks: packed must be contiguous (got strides %s)" % (tuple(packed.stride()),))
        L = int(packed.shape[0])
        nfun = 1 if packed.dim() == 2 else int(packed.shape[1])
        n = F if nfun == 1 else 2 * F
        if out is None:
            out = self.empty((L, n, n))
        if tuple(out.shape) != (L, n, n) or not out.is_contiguous():
            raise ValueError("Given output array is incompatible.")
        _check(self.lib.corahip_cl_blocks(self.h, self._f64(packed), L, nfun, F, self._f64(out)))
        return out

    # -- P(k) -> xi(r) (csrc/pk2xi.hip) --------------------------------------------------
    LOGCONV_MAX_LINE = 4096      # longest line of the FFT passes behind ``logconv``

    def _dev1d(self, t, name, n=None, dtype=None):
        """A contiguous 1-D device tensor of ``dtype`` (default float64) and, if given, length ``n``: its length."""
        torch = _torch()
        dtype = dtype or torch.float64
        if (not isinstance(t, torch.Tensor) or t.dim() != 1 or t.dtype != dtype or t.device != self.device
                or not t.is_contiguous() or (n is not None and t.numel() != n)):
            raise ValueError("%s must be a contiguous %s [%s] tensor on %s (got %r)"
                             % (name, str(dtype).replace("torch.", ""), "n" if n is None else n, self.device,
                                tuple(getattr(t, "shape", ()))))
        return int(t.numel())

    def sinc_romb(self, g, ka, dlk, r, out=None):
        """``out[j] = dlk * scipy.integrate.romb(g * sinc(ka * r[j]))`` (sinc(x) = sin x / x, 1 at 0) for ``g`` and ``ka``
        of ``2^k + 1`` samples, 1 <= k <= 24, and separations ``r`` [nr], all on the device.  With
        ``g = P(ka) ka^3 / 2 pi^2`` and ``dlk`` the logarithmic step of ``ka`` this is the reference's ``_corr_direct``.
        The summation order is fixed: the same call returns the same bits."""
        n = self._dev1d(g, "g")
        k = (n - 1).bit_length() - 1
        if n < 3 or n != (1 << k) + 1 or k > 24:
            raise ValueError("sinc_romb: g must have 2^k + 1 samples with 1 <= k <= 24 (got %d)" % n)
        self._dev1d(ka, "ka", n)
        nr = self._dev1d(r, "r")
        out = self._out_like(out, (nr,), "sinc_romb")
        for t, name in ((g, "g"), (ka, "ka"), (r, "r")):
            if self._overlap(out, nr * 8, t, t.numel() * 8):
                raise ValueError("sinc_romb: out overlaps %s" % name)
        _check(self.lib.corahip_sinc_romb(self.h, self._f64(g), self._f64(ka), k, float(dlk), self._f64(r), nr,
                                          self._f64(out)))
        return out

    def jl_romb(self, g, ka, dlk, r, lmask=None, out=None):
        """``out[s, i, j] = dlk * scipy.integrate.romb(g[s] * j_l(ka * r[j]))`` for ``l = 2 i`` = 0, 2, 4 (spherical Bessel
        functions) in one pass: ``g`` [nspec, 2^k + 1] with nspec 1 to 3 (or [2^k + 1]), ``ka`` [2^k + 1], ``r`` [nr] on the
        device -> [nspec, 3, nr].  ``lmask`` (host, one int per integrand, default 7): bit i set = order 2 i wanted; the
        other slots are +0.0.  The l = 0 slot has the bits of :meth:`sinc_romb`; a repeated call returns the same bits."""
        torch = _torch()
        if isinstance(g, torch.Tensor) and g.dim() == 1:
            g = g.unsqueeze(0)
        if (not isinstance(g, torch.Tensor) or g.dim() != 2 or g.dtype != torch.float64 or g.device != self.device
                or not g.is_contiguous()):
            raise ValueError("jl_romb: g must be a contiguous float64 [nspec, 2^k + 1] tensor on %s" % (self.device,))
        nspec, n = int(g.shape[0]), int(g.shape[1])
        k = (n - 1).bit_length() - 1
        if n < 3 or n != (1 << k) + 1 or k > 24:
            raise ValueError("jl_romb: g must have 2^k + 1 samples with 1 <= k <= 24 (got %d)" % n)
        if not 1 <= nspec <= 3:
            raise ValueError("jl_romb takes 1 to 3 integrands (got %d)" % nspec)
        masks = [7] * nspec if lmask is None else [int(m) for m in np.atleast_1d(lmask)]
        if len(masks) != nspec or any(m < 0 or m > 7 for m in masks):
            raise ValueError("jl_romb: lmask must hold one value 0 .. 7 per integrand (got %r)" % (lmask,))
        self._dev1d(ka, "ka", n)
        nr = self._dev1d(r, "r")
        out = self._out_like(out, (nspec, 3, nr), "jl_romb")
        for t, name in ((g, "g"), (ka, "ka"), (r, "r")):
            if self._overlap(out, out.numel() * 8, t, t.numel() * 8):
                raise ValueError("jl_romb: out overlaps %s" % name)
        _check(self.lib.corahip_jl_romb(self.h, self._f64(g), nspec, (c_int * nspec)(*masks), self._f64(ka), k, float(dlk),
                                        self._f64(r), nr, self._f64(out)))
        return out

    def xi_rsd(self, kx, ky, ky2, pi, sigma, coef, out=None):
        """``corahip_xi_rsd``: the redshift-space correlation function at the points (``pi``, ``sigma``) [n] from the
        multipole tables ``ky``, ``ky2`` [nfun, nk] (nfun 3: vv0 vv2 vv4; 6: + dd0 dv0 dv2) on the knots ``kx`` [nk] and
        the coefficient rows ``coef`` [ncoef, 4] = (b1 b2, (b1 f2 + b2 f1) / 2, f1 f2, D1 D2 pf1 pf2); point i reads row
        i % ncoef.  Everything on the device -> [n]."""
        nk = self._dev1d(kx, "kx")
        if ky.dim() != 2 or ky.shape[1] != nk or tuple(ky2.shape) != tuple(ky.shape):
            raise ValueError("xi_rsd: ky and ky2 must be [nfun, %d] (got %s, %s)" % (nk, tuple(ky.shape), tuple(ky2.shape)))
        if not (ky.is_contiguous() and ky2.is_contiguous()):
            raise ValueError("xi_rsd: ky and ky2 must be contiguous")
        nfun = int(ky.shape[0])
        if nfun not in (3, 6):
            raise ValueError("xi_rsd takes 3 tables (vv0 vv2 vv4) or 6 (+ dd0 dv0 dv2), got %d" % nfun)
        if nk < 4:
            raise ValueError("the spline tables need at least 4 knots (got %d)" % nk)
        n = self._dev1d(pi, "pi")
        self._dev1d(sigma, "sigma", n)
        if coef.dim() != 2 or coef.shape[1] != 4 or coef.shape[0] < 1 or not coef.is_contiguous():
            raise ValueError("xi_rsd: coef must be a contiguous [ncoef >= 1, 4] tensor (got %s)" % (tuple(coef.shape),))
        out = self._out_like(out, (n,), "xi_rsd")
        for t, name in ((pi, "pi"), (sigma, "sigma"), (coef, "coef"), (kx, "kx"), (ky, "ky"), (ky2, "ky2")):
            if self._overlap(out, n * 8, t, t.numel() * 8):
                raise ValueError("xi_rsd: out overlaps %s" % name)
        _check(self.lib.corahip_xi_rsd(self.h, self._f64(kx), self._f64(ky), self._f64(ky2), nk, nfun, self._f64(pi),
                                       self._f64(sigma), n, self._f64(coef), int(coef.shape[0]), self._f64(out)))
        return out

    def fftlog_phase(self, mu, L, N, out=None):
        """``U_m = exp(i (eta ln 2 + 2 Im lnGamma((mu + 1 + i eta) / 2)))``, ``eta = 2 pi m / L``, m = 0 .. N // 2: the
        unit-modulus FFTLog kernel at bias q = 0 as a complex128 device tensor [N // 2 + 1]."""
        torch = _torch()
        N, mu, L = int(N), float(mu), float(L)
        if N < 1 or not mu > -1.0 or not L > 0.0:
            raise ValueError("fftlog_phase needs N >= 1, mu > -1 and L > 0 (got N = %d, mu = %r, L = %r)" % (N, mu, L))
        if out is None:
            out = self.empty((N // 2 + 1,), dtype=torch.complex128)
        self._dev1d(out, "fftlog_phase: out", N // 2 + 1, torch.complex128)
        _check(self.lib.corahip_fftlog_phase(self.h, mu, L, N, self._c128(out)))
        return out

    @staticmethod
    def logconv_split(N):
        """``(N1, N2)`` with ``N1 * N2 == N`` that ``logconv`` takes: ``(N, 1)`` up to 4096 points, else the cheapest pair
        of divisors that are both at most 4096.  ValueError when N has none.  Needs no GPU."""
        N = int(N)
        if N < 1:
            raise ValueError("logconv_split: N must be positive (got %d)" % N)
        n1, n2 = c_int(0), c_int(0)
        if load().corahip_logconv_split(N, ctypes.byref(n1), ctypes.byref(n2)) != 0:
            raise ValueError("logconv: N = %d cannot be written as N1 * N2 with both factors <= %d (it has a prime factor "
                             "above %d or exceeds %d^2): choose samples_per_decade and the pads so that it can"
                             % (N, Context.LOGCONV_MAX_LINE, Context.LOGCONV_MAX_LINE, Context.LOGCONV_MAX_LINE))
        return int(n1.value), int(n2.value)

    def logconv(self, data, u, split=None):
        """In place ``data <- irfft(rfft(data.real) * u)``: the circular convolution of a real signal, held as a complex128
        device tensor [N] with zero imaginary parts, with the kernel whose half spectrum is ``u`` [N // 2 + 1].  On return
        the real parts are the result (natural order) and the imaginary parts rounding residue.  ``split`` = (N1, N2)
        chooses the four-step factorisation (default ``logconv_split(N)``); a unit factor means a single line transform."""
        torch = _torch()
        N = self._dev1d(data, "data", None, torch.complex128)
        if N < 1:
            raise ValueError("logconv: data is empty")
        self._dev1d(u, "u", N // 2 + 1, torch.complex128)
        n1, n2 = self.logconv_split(N) if split is None else (int(split[0]), int(split[1]))
        if n1 < 1 or n2 < 1 or n1 * n2 != N or max(n1, n2) > self.LOGCONV_MAX_LINE:
            raise ValueError("logconv: split %r does not factor N = %d into factors <= %d" % ((n1, n2), N, self.LOGCONV_MAX_LINE))
        if self._overlap(data, N * 16, u, u.numel() * 16):
            raise ValueError("logconv: data overlaps u")
        _check(self.lib.corahip_logconv(self.h, self._c128(data), self._c128(u), N, n1, n2))
        return data

    # -- n4: flat-sky fields -----------------------------------------------------------
    def _c128(self, t):
        torch = _torch()
        assert t.dtype == torch.complex128 and t.device == self.device
        return self._p(t)

    @staticmethod
    def _dims(shape):
        return (ctypes.c_int64 * len(shape))(*[int(x) for x in shape])

    def fft_c2c(self, data, axis, inverse=False):
        """In-place numpy.fft.fft / ifft of a complex128 device array along one axis."""
        axis = axis % data.dim()
        _check(self.lib.corahip_fft_c2c(self.h, self._c128(data), data.dim(), self._dims(data.shape), axis,
                                        1 if inverse else 0))
        return data

    def irfftn(self, spec, naxes=None, last=None):
        """numpy.fft.irfftn over the last ``naxes`` axes (default all); ``spec`` is overwritten."""
        nd = spec.dim()
        naxes = nd if naxes is None else naxes
        rshape = list(spec.shape)
        rshape[-1] = 2 * (spec.shape[-1] - 1) if last is None else int(last)
        if rshape[-1] // 2 + 1 != spec.shape[-1]:
            raise CoraHipError("irfftn: last axis %d does not match %d spectral bins" % (rshape[-1], spec.shape[-1]))
        out = self.empty(tuple(rshape))
        _check(self.lib.corahip_irfftn(self.h, self._c128(spec), nd, self._dims(rshape), naxes, self._f64(out)))
        return out

    def rfftn(self, arr, naxes=None):
        """numpy.fft.rfftn over the last ``naxes`` axes (default all) of a float64 device array."""
        torch = _torch()
        nd = arr.dim()
        naxes = nd if naxes is None else naxes
        cshape = list(arr.shape)
        cshape[-1] = arr.shape[-1] // 2 + 1
        spec = torch.empty(tuple(cshape), dtype=torch.complex128, device=self.device)
        _check(self.lib.corahip_rfftn(self.h, self._f64(arr), nd, self._dims(arr.shape), naxes, self._c128(spec)))
        return spec

    def randomfield_draw(self, kweight, seed):
        """(N(0,1) + i N(0,1)) * kweight from the Philox device stream (counter = flat element index)."""
        torch = _torch()
        spec = torch.empty(tuple(kweight.shape), dtype=torch.complex128, device=self.device)
        _check(self.lib.corahip_randomfield_draw(self.h, self._f64(kweight), kweight.numel(), int(seed),
                                                 self._c128(spec)))
        return spec

    def randomfield_irfftn(self, kweight, seed, last=None, spec=None):
        """``randomfield_draw`` + ``irfftn`` over all axes in one call: the spectrum is generated where the first pass
        loads it (same values, no separate draw pass).  kweight real [..., n/2 + 1]; returns the real field."""
        torch = _torch()
        nd = kweight.dim()
        rshape = list(kweight.shape)
        rshape[-1] = 2 * (kweight.shape[-1] - 1) if last is None else int(last)
        if rshape[-1] // 2 + 1 != kweight.shape[-1]:
            raise CoraHipError("randomfield_irfftn: last axis %d does not match %d spectral bins" % (rshape[-1], kweight.shape[-1]))
        if spec is None:
            spec = torch.empty(tuple(kweight.shape), dtype=torch.complex128, device=self.device)
        out = self.empty(tuple(rshape))
        _check(self.lib.corahip_randomfield_irfftn(self.h, self._f64(kweight), nd, self._dims(rshape), int(seed) & (2**64 - 1),
                                                   self._c128(spec), self._f64(out)))
        return out

    def fg_mix(self, freq_weight, normals, aff):
        """out[f] = aff * sum_c freq_weight[f, c] normals[c]  (complex [F, *aff.shape])."""
        torch = _torch()
        F, ncorr = freq_weight.shape
        assert normals.shape[0] == ncorr and tuple(normals.shape[1:]) == tuple(aff.shape)
        out = torch.empty((F,) + tuple(aff.shape), dtype=torch.complex128, device=self.device)
        _check(self.lib.corahip_fg_mix(self.h, self._f64(freq_weight), self._f64(normals), self._c128(aff), F, ncorr,
                                       aff.numel(), self._c128(out)))
        return out

    def spec_mul_real(self, spec, weight):
        assert tuple(spec.shape) == tuple(weight.shape)
        _check(self.lib.corahip_spec_mul_real(self.h, self._c128(spec), self._f64(weight), spec.numel()))
        return spec

    def cube_affine(self, df, vf, a, b, c):
        """out[z] = a[z] df[z] + b[z] vf[z] + c[z]; ``vf`` may be None."""
        n0 = df.shape[0]
        out = self.empty(tuple(df.shape))
        _check(self.lib.corahip_cube_affine(self.h, self._f64(df), None if vf is None else self._f64(vf), self._f64(a),
                                            None if vf is None else self._f64(b), self._f64(c), n0, df.numel() // n0,
                                            self._f64(out)))
        return out

    def raytrace_slices(self, cube, zc, scale, tx, ty, wx, wy):
        n0, n1, n2 = cube.shape
        numz, numx, numy = zc.numel(), tx.numel(), ty.numel()
        out = self.empty((numz, numx, numy))
        _check(self.lib.corahip_raytrace_slices(self.h, self._f64(cube), n0, n1, n2, self._f64(zc), self._f64(scale),
                                                self._f64(tx), self._f64(ty), float(wx), float(wy), numz, numx, numy,
                                                self._f64(out)))
        return out

    def healpix_neighbours(self, nside):
        """RING neighbour table [npix, 9] int32: the pixel itself, then healpy.get_all_neighbours' 8 (-1: none)."""
        torch = _torch()
        out = torch.empty((12 * int(nside) ** 2, 9), dtype=torch.int32, device=self.device)
        _check(self.lib.corahip_healpix_neighbours(self.h, int(nside), self._p(out)))
        return out

    def za_density_sph(self, psi, delta_bias, delta_m, chi, out, sigma_ang, sigma_chi):
        """Zel'dovich SPH assignment into ``out`` [nchi, npix] (added to, then minus 1); shapes checked by the caller."""
        nchi, npix = delta_bias.shape
        nside = int(round((npix // 12) ** 0.5))
        _check(self.lib.corahip_za_density_sph(self.h, self._f64(psi), self._f64(delta_bias), self._f64(delta_m),
                                               self._f64(chi), int(nchi), nside, float(sigma_ang), float(sigma_chi),
                                               self._f64(out)))
        return out

    # -- HEALPix bilinear interpolation (csrc/hpinterp.hip) -----------------------------------
    @staticmethod
    def _nside_of(npix):
        nside = int(round((int(npix) / 12.0) ** 0.5))
        if nside < 1 or 12 * nside * nside != int(npix):
            raise ValueError("Wrong pixel number (it is not 12*nside**2)")
        return nside

    def _directions(self, theta, phi):
        torch = _torch()
        if theta.dim() != 1 or tuple(phi.shape) != tuple(theta.shape):
            raise ValueError("theta and phi must be 1-d device tensors of one length")
        if theta.dtype != torch.float64 or phi.dtype != torch.float64:
            raise ValueError("theta and phi must be float64")
        if theta.device != self.device or phi.device != self.device:
            raise ValueError("theta and phi must be on %s" % (self.device,))
        return theta.contiguous(), phi.contiguous(), int(theta.shape[0])

    def _map_stack(self, maps):
        torch = _torch()
        if maps.dim() != 2 or maps.dtype != torch.float64 or not maps.is_contiguous() or maps.shape[0] < 1:
            raise ValueError("maps must be a contiguous float64 device tensor [n, npix], n >= 1")
        if maps.device != self.device:
            raise ValueError("maps must be on %s" % (self.device,))
        return int(maps.shape[0]), self._nside_of(maps.shape[1])

    def healpix_interp_weights(self, nside, theta, phi):
        """``healpy.get_interp_weights(nside, theta, phi)`` (RING) for 1-d float64 device tensors: ``(pix [4, n] int64,
        weights [4, n])`` on the device, the upper ring's two pixels first."""
        torch = _torch()
        theta, phi, n = self._directions(theta, phi)
        pix = torch.empty((4, n), dtype=torch.int64, device=self.device)
        w = self.empty((4, n))
        _check(self.lib.corahip_healpix_interp_weights(self.h, int(nside), self._f64(theta), self._f64(phi), n,
                                                       self._p(pix), self._f64(w)))
        return pix, w

    def healpix_interp_val(self, maps, theta, phi, out=None):
        """maps [nmap, npix] sampled at the directions -> [nmap, n]; weights once per direction, all maps in one launch."""
        nmap, nside = self._map_stack(maps)
        theta, phi, n = self._directions(theta, phi)
        if out is None:
            out = self.empty((nmap, n))
        elif (tuple(out.shape) != (nmap, n) or not out.is_contiguous() or out.dtype != maps.dtype
              or out.device != self.device):
            raise ValueError("out must be a contiguous float64 [%d, %d] tensor on %s" % (nmap, n, self.device))
        _check(self.lib.corahip_healpix_interp_val(self.h, self._f64(maps), nmap, nside, self._f64(theta), self._f64(phi),
                                                   n, self._f64(out)))
        return out

    def healpix_rotate_maps(self, maps, R, out=None):
        """``out[m, p] = interp(maps[m], R n_p)`` for the centre ``n_p`` of every pixel (R: host 3 x 3); ``out`` must not
        overlap ``maps`` (ValueError)."""
        nmap, nside = self._map_stack(maps)
        R = np.ascontiguousarray(R, dtype=np.float64)
        if R.shape != (3, 3):
            raise ValueError("R must be a 3 x 3 matrix (got shape %r)" % (R.shape,))
        if out is None:
            out = self.empty(tuple(maps.shape))
        elif (tuple(out.shape) != tuple(maps.shape) or not out.is_contiguous() or out.dtype != maps.dtype
              or out.device != self.device):
            raise ValueError("out must be a contiguous float64 tensor of the shape of maps on %s" % (self.device,))
        nbytes = maps.numel() * 8
        if self._overlap(out, nbytes, maps, nbytes):
            raise ValueError("healpix_rotate_maps: out overlaps maps")
        _check(self.lib.corahip_healpix_rotate_maps(self.h, self._f64(maps), nmap, nside,
                                                    R.ctypes.data_as(ctypes.POINTER(c_double)), self._f64(out)))
        return out

    def za_density_grid(self, psi, delta_bias, chi, out):
        """Zel'dovich grid assignment into ``out`` [nchi, npix] (added to, then minus 1); shapes checked by the caller."""
        nchi, npix = delta_bias.shape
        _check(self.lib.corahip_za_density_grid(self.h, self._f64(psi), self._f64(delta_bias), self._f64(chi), int(nchi),
                                                self._nside_of(npix), self._f64(out)))
        return out

    # -- polarised galaxy: Faraday-depth synthesis (csrc/faraday.hip) --------------------------------------------------
    def _cfield2d(self, t, name):
        torch = _torch()
        if not isinstance(t, torch.Tensor) or t.dim() != 2:
            raise ValueError("%s must be a 2-D complex128 device tensor (got shape %r)" % (name, tuple(getattr(t, "shape", ()))))
        if t.dtype != torch.complex128 or not t.is_contiguous() or t.device != self.device:
            raise ValueError("%s must be a contiguous complex128 tensor on %s" % (name, self.device))
        return int(t.shape[0]), int(t.shape[1])

    def complex_variance(self, y):
        """``chunk_var`` (cora/foreground/galaxy.py:58-83) of a complex128 device array: ``(var, mean)`` as a host float
        and complex, ``var = sum |y - mean|^2 / y.size``.  Fixed summation order (block partials, ordered final pass):
        identical bits from call to call.  Waits for the result."""
        torch = _torch()
        if not isinstance(y, torch.Tensor) or y.dtype != torch.complex128 or y.device != self.device:
            raise ValueError("complex_variance takes a complex128 tensor on %s" % (self.device,))
        if not y.is_contiguous() or y.numel() < 1:
            raise ValueError("complex_variance takes a contiguous, non-empty tensor")
        out = self.empty((3,))
        _check(self.lib.corahip_complex_variance(self.h, self._p(y), int(y.numel()), self._f64(out)))
        v = out.cpu().numpy()
        return float(v[0]), complex(v[1], v[2])

    def faraday_mix(self, y, phi, sigma, A, scale, intensity=None, out=None):
        """The fused depth -> frequency step of ``getpolsky`` (cora/foreground/galaxy.py:286-331), one FP64 MFMA kernel.

        y : complex128 device [ncol, nphi], the depth cube after the inverse FFT, unweighted; nphi even
        phi : [nphi] depth grid, sigma : [ncol] positive widths (host arrays or device tensors)
        A : complex128 [nfreq, nphi] (host or device), the transpose of the reference's ``pta``
        scale : float, ``1 / (2 sqrt(var))``

        ``w = exp(-0.25 (phi / sigma)^2)`` normalised over depth, ``z = scale * A @ (w y).T``, ``P = z tanh|z| / |z|``
        (0 where z = 0; the reference gives NaN there).  Returns P, complex128 [nfreq, ncol]; with ``intensity``
        (float64 device [nfreq, ncol]) returns float64 [nfreq, 4, ncol] = (intensity, Re P intensity, Im P intensity, 0).
        ``out`` must not overlap an input (ValueError).  No atomics: identical bits from call to call."""
        torch = _torch()
        ncol, nphi = self._cfield2d(y, "y")
        if nphi < 2 or nphi % 2 or ncol < 1:
            raise ValueError("faraday_mix: nphi must be even and >= 2 (got y of shape %r)" % ((ncol, nphi),))
        if isinstance(A, torch.Tensor):
            if A.dim() != 2:
                raise ValueError("A must be [nfreq, nphi] (got shape %r)" % (tuple(A.shape),))
        else:
            A = np.ascontiguousarray(A, dtype=np.complex128)
            if A.ndim != 2:
                raise ValueError("A must be [nfreq, nphi] (got shape %r)" % (A.shape,))
        nfreq = int(A.shape[0])
        if nfreq < 1 or int(A.shape[1]) != nphi:
            raise ValueError("Array A has the wrong shape (got %r, expected (nfreq, %d))" % (tuple(A.shape), nphi))
        for name, v, n in (("phi", phi, nphi), ("sigma", sigma, ncol)):
            if tuple(np.shape(v)) != (n,):
                raise ValueError("Array %s has shape %r, expected (%d,)" % (name, tuple(np.shape(v)), n))
        scale = float(scale)
        if intensity is not None:
            if (not isinstance(intensity, torch.Tensor) or tuple(intensity.shape) != (nfreq, ncol)
                    or intensity.dtype != torch.float64 or not intensity.is_contiguous() or intensity.device != self.device):
                raise ValueError("intensity must be a contiguous float64 [%d, %d] tensor on %s" % (nfreq, ncol, self.device))
            oshape, odtype = (nfreq, 4, ncol), torch.float64
        else:
            oshape, odtype = (nfreq, ncol), torch.complex128
        if out is not None and (not isinstance(out, torch.Tensor) or tuple(out.shape) != oshape or out.dtype != odtype
                                or not out.is_contiguous() or out.device != self.device):
            raise ValueError("out must be a contiguous %s %r tensor on %s" % (odtype, oshape, self.device))
        if not isinstance(A, torch.Tensor):
            A = torch.from_numpy(A).to(self.device)
        self._cfield2d(A, "A")
        phi = self._rowvec(phi, nphi, "phi")
        sigma = self._rowvec(sigma, ncol, "sigma")
        if out is None:
            out = torch.empty(oshape, dtype=odtype, device=self.device)
        obytes = out.numel() * out.element_size()
        for name, t in (("y", y), ("A", A), ("phi", phi), ("sigma", sigma), ("intensity", intensity)):
            if t is not None and self._overlap(out, obytes, t, t.numel() * t.element_size()):
                raise ValueError("faraday_mix: out overlaps %s" % name)
        _check(self.lib.corahip_faraday_mix(self.h, self._p(y), ncol, nphi, self._f64(phi), self._f64(sigma), self._p(A),
                                            nfreq, scale, None if intensity is None else self._f64(intensity),
                                            self._p(out)))
        return out

    def faraday_pack(self, maps, y, k0):
        """Real device maps ``[2 nchunk, npix]`` (rows 2 j, 2 j + 1: real and imaginary part of depth channel k0 + j) into
        columns ``k0 .. k0 + nchunk - 1`` of the complex128 depth cube ``y`` [npix, nphi] (an LDS tile transpose)."""
        torch = _torch()
        npix, nphi = self._cfield2d(y, "y")
        if (not isinstance(maps, torch.Tensor) or maps.dim() != 2 or maps.dtype != torch.float64 or not maps.is_contiguous()
                or maps.device != self.device):
            raise ValueError("maps must be a contiguous float64 [2 nchunk, npix] tensor on %s" % (self.device,))
        R = int(maps.shape[0])
        k0 = int(k0)
        if R < 2 or R % 2 or int(maps.shape[1]) != npix or k0 < 0 or k0 + R // 2 > nphi:
            raise ValueError("faraday_pack: maps %r at k0 = %d do not fit y %r" % (tuple(maps.shape), k0, (npix, nphi)))
        if self._overlap(y, npix * nphi * 16, maps, R * npix * 8):
            raise ValueError("faraday_pack: y overlaps maps")
        _check(self.lib.corahip_faraday_pack(self.h, self._f64(maps), R // 2, npix, k0, nphi, self._p(y)))
        return y

    # -- point sources (csrc/pointsource.hip) ---------------------------------------------------------------------------
    def _vec(self, v, n, name, dtype=None):
        """A host array or device tensor as a contiguous device vector of ``n`` elements (ValueError otherwise)."""
        torch = _torch()
        dtype = dtype or torch.float64
        if not isinstance(v, torch.Tensor):
            v = np.asarray(v)
            if v.shape != (n,):
                raise ValueError("%s has shape %r, expected (%d,)" % (name, v.shape, n))
            return torch.from_numpy(np.ascontiguousarray(v, dtype=np.int64 if dtype == torch.int64 else np.float64)).to(self.device)
        if tuple(v.shape) != (n,) or v.dtype != dtype or v.device != self.device or not v.is_contiguous():
            raise ValueError("%s must be a contiguous %s tensor of %d elements on %s" % (name, dtype, n, self.device))
        return v

    def pointsource_population(self, seed, n, knots, values, second, flux_min, spectral_mean, spectral_width, npix,
                               interval=False):
        """``n`` synthetic sources in one launch: ``(pix int64 [n], flux [n], index [n])`` device tensors (and the int32
        spline interval and float64 spline value of every source with ``interval=True``).  ``knots, values, second``: the inverse-CDF spline
        (``Interpolater.data()``), host arrays.  The mapping from ``(seed, i)`` to source i is written down in
        include/corahip.h and tests/_pointsource_oracle.py."""
        torch = _torch()
        n, npix = int(n), int(npix)
        knots = np.ascontiguousarray(knots, dtype=np.float64)
        if knots.ndim != 1 or knots.size < 2:
            raise ValueError("knots must be a 1-d array of at least 2 elements")
        if n < 0 or npix < 1:
            raise ValueError("pointsource_population: n >= 0 and npix >= 1 (got %d, %d)" % (n, npix))
        if not (knots[0] <= 0.0 and knots[-1] >= 1.0 and np.all(np.diff(knots) >= 0)):
            raise ValueError("knots must ascend from 0 to 1 (an inverse CDF)")
        xs = self._vec(knots, knots.size, "knots")
        ys, y2 = self._vec(values, knots.size, "values"), self._vec(second, knots.size, "second")
        pix = torch.empty((n,), dtype=torch.int64, device=self.device)
        flux, index = self.empty((n,)), self.empty((n,))
        iv = torch.empty((n,), dtype=torch.int32, device=self.device) if interval else None
        sv = self.empty((n,)) if interval else None
        _check(self.lib.corahip_pointsource_population(self.h, c_u64(int(seed) & (2**64 - 1)), n, self._f64(xs), self._f64(ys),
                                                       self._f64(y2), int(knots.size), float(flux_min), float(spectral_mean),
                                                       float(spectral_width), npix, self._p(pix), self._f64(flux),
                                                       self._f64(index), self._p0(iv), self._p0(sv)))
        return (pix, flux, index, iv, sv) if interval else (pix, flux, index)

    def pointsource_paint(self, pix, flux, beta, x, den, c2, npix, gamma=None, polw=None, npol=1, out=None, accumulate=False):
        """Sources sorted by pixel painted into ``out`` [nfreq, npol, npix] (``npol`` 1: [nfreq, npix]):
        ``out[f, 0, p] (+)= ((sum_i flux_i exp(beta_i x_f + gamma_i x_f^2)) 1e-26 c2) / den_f`` over the sources of pixel p,
        planes 1, 2 the same sums weighted by ``polw[:, 0 / 1]``.  ``pix`` int64 ascending in [0, npix) (the caller
        sorts); ``x``, ``den`` host arrays [nfreq].  One writer per element, fixed summation order, no atomics: identical
        bits from call to call and for any subset of channels.  ``accumulate``: add to ``out`` (occupied pixels only)
        instead of writing all of it."""
        torch = _torch()
        if not isinstance(pix, torch.Tensor) or pix.dim() != 1:
            raise ValueError("pix must be a 1-d int64 device tensor")
        n, npix, npol = int(pix.shape[0]), int(npix), int(npol)
        if npol not in (1, 4) or (polw is not None and npol != 4):
            raise ValueError("npol must be 1 or 4, and 4 with polw")
        x = np.ascontiguousarray(x, dtype=np.float64)
        den = np.ascontiguousarray(den, dtype=np.float64)
        if x.ndim != 1 or x.size < 1 or den.shape != x.shape:
            raise ValueError("x and den must be 1-d arrays of one length (got %r, %r)" % (x.shape, den.shape))
        F = int(x.size)
        pix = self._vec(pix, n, "pix", torch.int64)
        flux, beta = self._vec(flux, n, "flux"), self._vec(beta, n, "beta")
        gamma = None if gamma is None else self._vec(gamma, n, "gamma")
        if polw is not None:
            if not isinstance(polw, torch.Tensor):
                polw = self.to_device(np.asarray(polw, dtype=np.float64))
            if tuple(polw.shape) != (n, 2) or polw.dtype != torch.float64 or polw.device != self.device or not polw.is_contiguous():
                raise ValueError("polw must be a contiguous float64 [%d, 2] tensor on %s" % (n, self.device))
        shape = (F, npix) if npol == 1 else (F, npol, npix)
        if out is None:
            if accumulate:
                raise ValueError("accumulate needs out")
            out = self.empty(shape)
        elif (not isinstance(out, torch.Tensor) or tuple(out.shape) != shape or out.dtype != torch.float64
              or out.device != self.device or not out.is_contiguous()):
            raise ValueError("out must be a contiguous float64 %r tensor on %s" % (shape, self.device))
        xd, dend = self.to_device(x), self.to_device(den)     # named: they must outlive the argument list
        _check(self.lib.corahip_pointsource_paint(self.h, n, self._p(pix), self._f64(flux), self._f64(beta), self._p0(gamma),
                                                  self._p0(polw), self._f64(xd), self._f64(dend), float(c2), F, npol, npix,
                                                  1 if accumulate else 0, self._f64(out)))
        return out

    def _cube(self, t, rank, name):
        torch = _torch()
        if (not isinstance(t, torch.Tensor) or t.dim() != rank or t.dtype != torch.float64 or t.device != self.device
                or not t.is_contiguous() or t.numel() < 1):
            raise ValueError("%s must be a contiguous, non-empty float64 device tensor of rank %d on %s" % (name, rank, self.device))
        return t

    def polarise_rotate(self, intensity, qfrac, ufrac, wv=None, rm=None, out=None):
        """``intensity`` [nfreq, npix] -> [nfreq, 4, npix] = (I, Re P, Im P, 0), ``P = I (qfrac + i ufrac) exp(-2i wv_f rm_p)``
        (pointsource.py:258-276); ``rm=None``: no rotation.  ``wv`` [nfreq] host array, the wavelength ``1e-6 c / freq``."""
        intensity = self._cube(intensity, 2, "intensity")
        F, npix = int(intensity.shape[0]), int(intensity.shape[1])
        q, u = self._vec(qfrac, npix, "qfrac"), self._vec(ufrac, npix, "ufrac")
        rmd = None if rm is None else self._vec(rm, npix, "rm")
        if rm is not None and wv is None:
            raise ValueError("polarise_rotate: rm needs wv")
        wvd = None if wv is None else self._vec(np.asarray(wv, dtype=np.float64), F, "wv")
        if out is None:
            out = self.empty((F, 4, npix))
        elif self._cube(out, 3, "out").shape != (F, 4, npix):
            raise ValueError("out must be [%d, 4, %d]" % (F, npix))
        _check(self.lib.corahip_polarise_rotate(self.h, self._f64(intensity), self._f64(q), self._f64(u), self._p0(rmd),
                                                self._p0(wvd), F, npix, self._f64(out)))
        return out

    def faraday_rotate(self, polmap, rm, wv):
        """``faraday_rotate`` (pointsource.py:21-51) in place on the device cube ``polmap`` [nfreq, npol >= 3, npix]."""
        polmap = self._cube(polmap, 3, "polmap")
        F, npol, npix = (int(v) for v in polmap.shape)
        if npol < 3:
            raise ValueError("polmap needs the planes T, Q, U (got %d planes)" % npol)
        rmd = self._vec(rm, npix, "rm")
        wvd = self._vec(np.asarray(wv, dtype=np.float64), F, "wv")
        _check(self.lib.corahip_faraday_rotate(self.h, self._f64(polmap), self._f64(rmd), self._f64(wvd), F, npol, npix))
        return polmap

    def healpix_ud_grade(self, maps, nside_out):
        """``healpy.ud_grade(power=None)`` of device maps [nmap, npix], RING in and out: [nmap, 12 nside_out^2]."""
        nmap, nside_in = self._map_stack(maps)
        nside_out = int(nside_out)
        for ns in (nside_in, nside_out):
            if ns < 1 or ns & (ns - 1) or ns > 8192:
                raise ValueError("ud_grade: nside must be a power of two up to 8192 (got %d)" % ns)
        if nside_in > 64 * nside_out:
            raise ValueError("ud_grade degrades by at most a factor 64 in nside per call (got %d -> %d)" % (nside_in, nside_out))
        out = self.empty((nmap, 12 * nside_out * nside_out))
        _check(self.lib.corahip_healpix_ud_grade(self.h, self._f64(maps), nmap, nside_in, nside_out, self._f64(out)))
        return out

    # -- constrained galaxy (csrc/galaxy.hip) ----------------------------------------------------------------------------
    def _out_like(self, out, shape, name):
        torch = _torch()
        if out is None:
            return self.empty(shape)
        if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != torch.float64
                or out.device != self.device or not out.is_contiguous()):
            raise ValueError("%s: out must be a contiguous float64 %r tensor on %s" % (name, tuple(shape), self.device))
        return out

    def healpix_reorder(self, maps, r2n, out=None):
        """``healpy.reorder`` of device maps [nmap, npix]: RING -> NESTED with ``r2n`` true, NESTED -> RING otherwise.  A
        gather with the pixel map computed in the kernel; ``out`` must not overlap ``maps`` (ValueError)."""
        nmap, nside = self._map_stack(maps)
        if nside & (nside - 1) or nside > 8192:
            raise ValueError("healpix_reorder: nside must be a power of two up to 8192 (got %d)" % nside)
        out = self._out_like(out, maps.shape, "healpix_reorder")
        nbytes = maps.numel() * 8
        if self._overlap(out, nbytes, maps, nbytes):
            raise ValueError("healpix_reorder: out overlaps maps")
        _check(self.lib.corahip_healpix_reorder(self.h, self._f64(maps), nmap, nside, 1 if r2n else 0, self._f64(out)))
        return out

    def healpix_block_variance(self, maps, nside_out):
        """``map_variance`` (cora/foreground/galaxy.py:43-55) of device maps [nmap, npix]: [nmap, 12 nside_out^2], the
        variance (numpy ``var``, ddof 0) of the children of every RING pixel at ``nside_out``.  Two passes, pairwise sums in
        NESTED child order."""
        nmap, nside_in = self._map_stack(maps)
        nside_out = int(nside_out)
        for ns in (nside_in, nside_out):
            if ns < 1 or ns & (ns - 1) or ns > 8192:
                raise ValueError("block_variance: nside must be a power of two up to 8192 (got %d)" % ns)
        if nside_out > nside_in:
            raise ValueError("block_variance: nside_out must not exceed the maps' nside (got %d -> %d)" % (nside_in, nside_out))
        if nside_in > 64 * nside_out:
            raise ValueError("block_variance takes at most a factor 64 in nside per call (got %d -> %d)" % (nside_in, nside_out))
        out = self.empty((nmap, 12 * nside_out * nside_out))
        _check(self.lib.corahip_healpix_block_variance(self.h, self._f64(maps), nmap, nside_in, nside_out, self._f64(out)))
        return out

    def alm_scale_l(self, alm, lmax, fl, out=None):
        """a_lm in the device layout [nalm, G, 2, 4] times ``fl[channel, l]``: ``fl`` [nnu, lmax + 1] with
        ``4 (G - 1) < nnu <= 4 G``, or [lmax + 1] for all ``4 G`` channels (host array or device tensor).  One multiply per
        component; padding channels are copied.  ``out`` may be ``alm`` itself (in place) but not overlap it in part."""
        torch = _torch()
        lmax = int(lmax)
        nalm = (lmax + 1) * (lmax + 2) // 2
        if (not isinstance(alm, torch.Tensor) or alm.dim() != 4 or alm.shape[0] != nalm or tuple(alm.shape[2:]) != (2, 4)
                or alm.dtype != torch.float64 or alm.device != self.device or not alm.is_contiguous() or alm.shape[1] < 1):
            raise ValueError("alm must be a contiguous float64 [%d, G, 2, 4] tensor on %s" % (nalm, self.device))
        G = int(alm.shape[1])
        if not isinstance(fl, torch.Tensor):
            fl = self.to_device(np.asarray(fl, dtype=np.float64))
        if fl.dtype != torch.float64 or fl.device != self.device:
            raise ValueError("fl must be float64 on %s" % (self.device,))
        if fl.dim() == 1 and fl.shape[0] == lmax + 1:
            fl = fl[None, :].expand(4 * G, lmax + 1)
        if fl.dim() != 2 or fl.shape[1] != lmax + 1 or not 4 * (G - 1) < fl.shape[0] <= 4 * G:
            raise ValueError("fl must be [lmax + 1] or [nnu, lmax + 1] with %d < nnu <= %d (got %r)"
                             % (4 * (G - 1), 4 * G, tuple(fl.shape)))
        fl = fl.contiguous()
        nnu = int(fl.shape[0])
        out = alm if out is alm else self._out_like(out, alm.shape, "alm_scale_l")
        nbytes = alm.numel() * 8
        if out.data_ptr() != alm.data_ptr() and self._overlap(out, nbytes, alm, nbytes):
            raise ValueError("alm_scale_l: out overlaps alm in part")
        _check(self.lib.corahip_alm_scale_l(self.h, self._f64(alm), lmax, nnu, self._f64(fl), self._f64(out)))
        return out

    def galaxy_combine(self, fg, fgs, haslam, sc, am, mv, efreq, skip=2, out=None):
        """The end of ``ConstrainedGalaxy.getsky`` (cora/foreground/galaxy.py:181-198) in one launch: [nchan - skip, npix],
        ``S (1 + tanh_lin(((am / mv) (fg - fgs)) / S))`` with ``S = haslam (efreq / 408)^sc`` for the channels from ``skip``.

        fg, fgs : device [nchan, npix]; haslam, sc, am : [npix] (host arrays or device tensors); efreq : host [nchan] in
        MHz; mv : host float.  ``haslam`` and ``mv`` must be finite and positive (the reference gives NaN otherwise) and
        ``|sc log(efreq / 408)| < 512``: ValueError before the launch."""
        torch = _torch()
        fg, fgs = self._cube(fg, 2, "fg"), self._cube(fgs, 2, "fgs")
        nchan, npix = int(fg.shape[0]), int(fg.shape[1])
        self._nside_of(npix)
        if tuple(fgs.shape) != (nchan, npix):
            raise ValueError("fgs has shape %r, expected %r" % (tuple(fgs.shape), (nchan, npix)))
        skip = int(skip)
        if not 0 <= skip < nchan:
            raise ValueError("skip must be in [0, %d) (got %d)" % (nchan, skip))
        efreq = np.asarray(efreq, dtype=np.float64)
        if efreq.shape != (nchan,) or not (np.all(np.isfinite(efreq)) and np.all(efreq > 0)):
            raise ValueError("efreq must hold %d finite, positive frequencies" % nchan)
        mv = float(mv)
        if not (np.isfinite(mv) and mv > 0 and np.isfinite(1.0 / mv)):
            raise ValueError("mv must be finite and positive (got %r)" % mv)
        haslam, sc, am = self._vec(haslam, npix, "haslam"), self._vec(sc, npix, "sc"), self._vec(am, npix, "am")
        if not bool((torch.isfinite(haslam) & (haslam > 0)).all()):
            raise ValueError("haslam must be finite and positive")
        lnr = np.log(efreq / 408.0)
        if not float(sc.abs().max()) * float(np.abs(lnr).max()) < 512.0:      # (NaN fails too)
            raise ValueError("sc: |sc log(efreq / 408)| must stay below 512")
        out = self._out_like(out, (nchan - skip, npix), "galaxy_combine")
        obytes = out.numel() * 8
        for t, name in ((fg, "fg"), (fgs, "fgs"), (haslam, "haslam"), (sc, "sc"), (am, "am")):
            if self._overlap(out, obytes, t, t.numel() * 8):
                raise ValueError("galaxy_combine: out overlaps %s" % name)
        if out.data_ptr() % 16:
            raise ValueError("galaxy_combine: out must be 16-byte aligned")
        fg, fgs, haslam, sc, am = (t if t.data_ptr() % 16 == 0 else t.clone() for t in (fg, fgs, haslam, sc, am))
        lnrd = self.to_device(lnr)
        _check(self.lib.corahip_galaxy_combine(self.h, self._f64(fg), self._f64(fgs), self._f64(haslam), self._f64(sc),
                                               self._f64(am), 1.0 / mv, self._f64(lnrd), nchan, skip, npix, self._f64(out)))
        return out

    # -- LOFAR synchrotron (csrc/lofar.hip) --------------------------------------------------------------------------------
    def _depth_field(self, f, name):
        """A contiguous float64 device field [..., nz] with at least two axes: (ncol, nz), ncol the product of the others."""
        torch = _torch()
        if (not isinstance(f, torch.Tensor) or f.dim() < 2 or f.dtype != torch.float64 or f.device != self.device
                or not f.is_contiguous() or f.numel() < 1):
            raise ValueError("%s must be a contiguous, non-empty float64 [..., nz] tensor on %s (got %r)"
                             % (name, self.device, tuple(getattr(f, "shape", ()))))
        nz = int(f.shape[-1])
        return int(f.numel()) // nz, nz

    @staticmethod
    def powerlaw_range_check(xmax, b0, sb, beta_absmax):
        """The guard of ``powerlaw_los`` (that of ``galaxy_combine``): ValueError unless ``xmax (|b0| + |sb| beta_absmax) <
        512``, the range of the kernel's exp.  Host arithmetic only."""
        if not float(xmax) * (abs(float(b0)) + abs(float(sb)) * float(beta_absmax)) < 512.0:      # (NaN fails too)
            raise ValueError("powerlaw_los: |x (b0 + sb beta)| must stay below 512")

    def field_moments(self, f):
        """``(f.sum(axis=-1).std(), f.std(), abs(f).max())`` of a device field [..., nz] as host floats (numpy's ``ddof = 0``):
        two passes each, fixed summation order, identical bits from call to call.  Waits for the result."""
        ncol, nz = self._depth_field(f, "f")
        out = self.empty((3,))
        _check(self.lib.corahip_field_moments(self.h, self._f64(f), ncol, nz, self._f64(out)))
        v = out.cpu().numpy()
        return float(v[0]), float(v[1]), float(v[2])

    def powerlaw_los(self, A, beta, x, a0=0.0, sa=1.0, b0=0.0, sb=1.0, out=None, beta_absmax=None):
        """``out[i, p] = sum_z (a0 + sa A[p, z]) exp(x[i] (b0 + sb beta[p, z]))`` in one launch: [nfreq, ncol], ncol the
        product of all axes of the fields but the last.

        A, beta : device fields [..., nz] of one shape (``beta is A`` is allowed); x : [nfreq], host array or device
        tensor, ``log(nu / nu_0)``; beta_absmax : ``max |beta|`` if the caller has it (``field_moments``), else it is
        measured here.  ``max|x| (|b0| + |sb| max|beta|) < 512`` (the range of the kernel's exp): ValueError before the
        launch otherwise.  The depth sum runs in the order of z whatever ``x`` holds: a subset of the channels gives the
        bits those channels have in the full call."""
        torch = _torch()
        ncol, nz = self._depth_field(A, "A")
        if beta is not A and (self._depth_field(beta, "beta") != (ncol, nz) or beta.shape != A.shape):
            raise ValueError("beta has shape %r, expected %r" % (tuple(beta.shape), tuple(A.shape)))
        if not isinstance(x, torch.Tensor):
            x = self.to_device(np.asarray(x, dtype=np.float64).reshape(-1))
        if x.dim() != 1 or x.numel() < 1 or x.dtype != torch.float64 or x.device != self.device or not x.is_contiguous():
            raise ValueError("x must be a non-empty float64 vector")
        nfreq = int(x.numel())
        a0, sa, b0, sb = float(a0), float(sa), float(b0), float(sb)
        if not all(np.isfinite(v) for v in (a0, sa, b0, sb)):
            raise ValueError("powerlaw_los: a0, sa, b0, sb must be finite (got %r)" % ((a0, sa, b0, sb),))
        bmax = float(self.field_moments(beta)[2] if beta_absmax is None else beta_absmax)
        self.powerlaw_range_check(float(x.abs().max()), b0, sb, bmax)
        out = self._out_like(out, (nfreq, ncol), "powerlaw_los")
        obytes = out.numel() * 8
        for t, name in ((A, "A"), (beta, "beta"), (x, "x")):
            if self._overlap(out, obytes, t, t.numel() * 8):
                raise ValueError("powerlaw_los: out overlaps %s" % name)
        _check(self.lib.corahip_powerlaw_los(self.h, self._f64(A), self._f64(beta), self._f64(x), a0, sa, b0, sb, nfreq, ncol,
                                             nz, self._f64(out)))
        return out

    # -- exact curved-sky C_l (csrc/fullsky.hip) ---------------------------------------------------------------------------
    FULLSKY_MAX_NSUB = 17

    def _fullsky_args(self, k, chi, cb, cf, lmax, name):
        """(k [nk], chi, cb, cf [F, nsub]) as contiguous float64 device tensors, from host arrays or device tensors."""
        torch = _torch()

        def dev(a, nm):
            if not isinstance(a, torch.Tensor):
                a = self.to_device(np.asarray(a, dtype=np.float64))
            if a.dtype != torch.float64 or a.device != self.device:
                raise ValueError("%s: %s must be float64 on %s" % (name, nm, self.device))
            return a.contiguous()

        k, chi, cb, cf = dev(k, "k"), dev(chi, "chi"), dev(cb, "cb"), dev(cf, "cf")
        if chi.dim() == 1:
            chi, cb, cf = chi[:, None], cb[:, None] if cb.dim() == 1 else cb, cf[:, None] if cf.dim() == 1 else cf
        if k.dim() != 1 or k.numel() < 1 or chi.dim() != 2 or cb.shape != chi.shape or cf.shape != chi.shape:
            raise ValueError("%s: k must be [nk], chi, cb, cf of one shape [F, nsub] (got %r, %r, %r, %r)"
                             % (name, tuple(k.shape), tuple(chi.shape), tuple(cb.shape), tuple(cf.shape)))
        F, nsub = int(chi.shape[0]), int(chi.shape[1])
        if F < 1 or F > 65535 or nsub < 1 or nsub > self.FULLSKY_MAX_NSUB:
            raise ValueError("%s: 1 <= F <= 65535 and 1 <= nsub <= %d (got F = %d, nsub = %d)"
                             % (name, self.FULLSKY_MAX_NSUB, F, nsub))
        if int(lmax) != lmax or lmax < 0:
            raise ValueError("%s: lmax must be a non-negative integer (got %r)" % (name, lmax))
        return k, chi.contiguous(), cb.contiguous(), cf.contiguous(), F, nsub, int(lmax)

    def sphbessel_radial(self, k, chi, cb, cf, lmax, ld_k=None):
        """The radial table ``A[l, i, n] = sum_a cb[i, a] j_l(k_n chi[i, a]) - cf[i, a] j_l''(k_n chi[i, a])`` for
        ``l = 0 .. lmax`` as a ``[lmax + 1, F, nk]`` device tensor (``corahip_sphbessel_radial``).

        k : [nk] wavenumbers (>= 0, finite); chi, cb, cf : [F, nsub] (or [F]), the sub-samples of each channel with their
        weights; host arrays or device tensors.  With ``ld_k > nk`` the result is the view ``[..., :nk]`` of a
        ``[lmax + 1, F, ld_k]`` tensor whose other columns are zero.  j_l comes from the upward recurrence below the turning
        point and a normalised downward one above it; the values are finite for every finite ``k chi >= 0`` and the same
        from call to call."""
        k, chi, cb, cf, F, nsub, lmax = self._fullsky_args(k, chi, cb, cf, lmax, "sphbessel_radial")
        nk = int(k.numel())
        ld = nk if ld_k is None else int(ld_k)
        if ld < nk:
            raise ValueError("sphbessel_radial: ld_k must be >= nk")
        A = self.empty((lmax + 1, F, ld))
        _check(self.lib.corahip_sphbessel_radial(self.h, self._f64(k), nk, self._f64(chi), self._f64(cb), self._f64(cf), F,
                                                 nsub, lmax, ld, self._f64(A)))
        return A if ld == nk else A[:, :, :nk]

    def cl_gram(self, A, g, out=None, accumulate=False):
        """``C[l, i, j] = sum_n g_n A[l, i, n] A[l, j, n]`` (added to ``out`` with ``accumulate``) as ``[nl, F, F]``: one
        FP64 MFMA Gram product per l (``corahip_cl_gram``).

        A : float64 device tensor [nl, F, nk], k contiguous; a view ``[..., :nk]`` of a wider tensor is taken as it is.
        g : [nk], either sign.  The result equals its transpose bit for bit; the sum of an element runs over n in ascending
        order whatever F is, so the rows of a subset of the channels give the bits of the full result's sub-block."""
        torch = _torch()
        if not isinstance(A, torch.Tensor) or A.dim() != 3 or A.dtype != torch.float64 or A.device != self.device or A.numel() < 1:
            raise ValueError("cl_gram: A must be a non-empty float64 [nl, F, nk] tensor on %s" % (self.device,))
        nl, F, nk = (int(v) for v in A.shape)
        ld = int(A.stride(1)) if F > 1 else (int(A.stride(0)) if nl > 1 else nk)
        if (nk > 1 and A.stride(2) != 1) or ld < nk or (nl > 1 and A.stride(0) != F * ld):
            A = A.contiguous()
            ld = nk
        if not isinstance(g, torch.Tensor):
            g = self.to_device(np.asarray(g, dtype=np.float64))
        if g.dtype != torch.float64 or g.device != self.device or tuple(g.shape) != (nk,):
            raise ValueError("cl_gram: g must be float64 [%d]" % nk)
        g = g.contiguous()
        if accumulate and out is None:
            raise ValueError("cl_gram: accumulate needs out")
        out = self._out_like(out, (nl, F, F), "cl_gram")
        if self._overlap(out, out.numel() * 8, A, ((nl * F - 1) * ld + nk) * 8):
            raise ValueError("cl_gram: out overlaps A")
        _check(self.lib.corahip_cl_gram(self.h, c_void_p(A.data_ptr()), self._f64(g), nl - 1, F, nk, ld, self._f64(out),
                                        1 if accumulate else 0))
        return out

    def clarray_fullsky_chunk(self, lmax, F, nk, max_bytes=None):
        """The number of wavenumbers per pass of :meth:`clarray_fullsky` under a workspace budget of ``max_bytes`` (default:
        a quarter of the device memory, at most 16 GiB): a multiple of 16, at least 16, no more than nk rounded up."""
        torch = _torch()
        if max_bytes is None:
            max_bytes = min(torch.cuda.get_device_properties(self.device).total_memory // 4, 16 << 30)
        per = 8 * (int(lmax) + 1) * int(F)
        chunk = max(int(max_bytes) // per // 16 * 16, 16)
        return min(chunk, (int(nk) + 15) // 16 * 16)

    def clarray_fullsky(self, k, g, chi, cb, cf, lmax, max_bytes=None, nk_chunk=None):
        """``C[l, i, j] = sum_n g_n A_l[i, n] A_l[j, n]`` with the radial table of :meth:`sphbessel_radial`, as a
        ``[lmax + 1, F, F]`` device tensor (``corahip_clarray_fullsky``).  The k axis runs in ascending chunks whose table
        fits ``max_bytes`` (:meth:`clarray_fullsky_chunk`; ``nk_chunk`` sets the length itself): table, then Gram product,
        accumulating after the first.  Symmetric bit for bit, the same bits from call to call."""
        torch = _torch()
        k, chi, cb, cf, F, nsub, lmax = self._fullsky_args(k, chi, cb, cf, lmax, "clarray_fullsky")
        nk = int(k.numel())
        if not isinstance(g, torch.Tensor):
            g = self.to_device(np.asarray(g, dtype=np.float64))
        if g.dtype != torch.float64 or g.device != self.device or tuple(g.shape) != (nk,):
            raise ValueError("clarray_fullsky: g must be float64 [%d]" % nk)
        g = g.contiguous()
        chunk = self.clarray_fullsky_chunk(lmax, F, nk, max_bytes) if nk_chunk is None else int(nk_chunk)
        if chunk < 1:
            raise ValueError("clarray_fullsky: nk_chunk must be positive")
        b = c_size_t()
        _check(self.lib.corahip_clarray_fullsky_workspace_bytes(lmax, F, chunk, ctypes.byref(b)))
        work = torch.empty(int(b.value) // 8, dtype=torch.float64, device=self.device)
        out = self.empty((lmax + 1, F, F))
        _check(self.lib.corahip_clarray_fullsky(self.h, self._f64(k), self._f64(g), nk, self._f64(chi), self._f64(cb),
                                                self._f64(cf), F, nsub, lmax, chunk, self._p(work), self._f64(out)))
        return out

    # -- mkconstrained (csrc/constrained.hip) ------------------------------------------------------------------------------
    EIG_TOP_MAX_K = 8

    def _stack3(self, t, name, last=None):
        """A contiguous float64 device tensor [n, F, last]: (n, F, last)."""
        torch = _torch()
        if (not isinstance(t, torch.Tensor) or t.dim() != 3 or t.dtype != torch.float64 or t.device != self.device
                or not t.is_contiguous() or min(t.shape) < 1 or (last is not None and t.shape[2] != last)):
            raise ValueError("%s must be a contiguous float64 [n, F, %s] tensor on %s (got %r)"
                             % (name, "F" if last is None else last, self.device, tuple(getattr(t, "shape", ()))))
        return tuple(int(s) for s in t.shape)

    def eig_top_max_f(self):
        """Most channels ``eig_top_batched`` takes: its two F x 16 blocks live in the LDS of one workgroup."""
        n = c_int(0)
        _check(self.lib.corahip_eig_top_max_f(self.h, ctypes.byref(n)))
        return int(n.value)

    def eig_top_batched(self, C, k, max_iter=None, out=None):
        """The ``k`` algebraically largest eigenpairs of every symmetric ``C[l]`` (device [L, F, F], lower triangle read):
        ``(V, theta, info)`` with V [L, F, k] as ``scipy.linalg.eigh(C[l])[1][:, -k:]`` up to the signs of the columns,
        theta [L, k] ascending, info [L] int32: 0 = block orthogonal iteration, 1 = full Jacobi decomposition (a block
        that has not met the stop rule ``|C v - theta v| <= 8 F u |C|_inf`` after ``max_iter`` products; default: the
        library's).  ``1 <= k <= min(8, F)``, ``F <= eig_top_max_f()``.  ``out``: optional ``(V, theta, info)`` to fill."""
        torch = _torch()
        L, F, F2 = self._stack3(C, "C")
        if F2 != F:
            raise ValueError("C must be [L, F, F] (got %r)" % (tuple(C.shape),))
        k = int(k)
        if not 1 <= k <= min(self.EIG_TOP_MAX_K, F):
            raise ValueError("eig_top_batched: k must be in 1 .. min(%d, F = %d) (got %d)" % (self.EIG_TOP_MAX_K, F, k))
        max_iter = 0 if max_iter is None else int(max_iter)
        if max_iter < 0:
            raise ValueError("eig_top_batched: max_iter must be positive (got %d)" % max_iter)
        if out is None:
            V, theta = self.empty((L, F, k)), self.empty((L, k))
            info = torch.empty((L,), dtype=torch.int32, device=self.device)
        else:
            V, theta, info = out
            V, theta = self._out_like(V, (L, F, k), "eig_top_batched"), self._out_like(theta, (L, k), "eig_top_batched")
            if (not isinstance(info, torch.Tensor) or tuple(info.shape) != (L,) or info.dtype != torch.int32
                    or info.device != self.device or not info.is_contiguous()):
                raise ValueError("eig_top_batched: info must be a contiguous int32 [%d] tensor on %s" % (L, self.device))
            ts = ((C, "C"), (V, "V"), (theta, "theta"), (info, "info"))
            for i in range(1, 4):
                for j in range(i):
                    a, b = ts[i][0], ts[j][0]
                    if self._overlap(a, a.numel() * a.element_size(), b, b.numel() * b.element_size()):
                        raise ValueError("eig_top_batched: %s overlaps %s" % (ts[i][1], ts[j][1]))
        fmax = self.eig_top_max_f()
        if F > fmax:
            raise ValueError("eig_top_batched: F = %d channels exceed the limit of %d" % (F, fmax))
        _check(self.lib.corahip_eig_top_batched(self.h, self._f64(C), L, F, k, max_iter, self._f64(V), self._f64(theta),
                                                self._p(info)))
        return V, theta, info

    def constrained_weights(self, V, f_ind):
        """``W[l] = V[l] (V[l][f_ind, :])^-1`` for device V [L, F, k] (``eig_top_batched``) and the ``k`` constrained
        channels ``f_ind`` (host integers): W [L, F, k], the weights that carry the constraint a_lm to all channels
        (cora/core/skysim.py:180-194).  ``W[0] = 0`` whatever ``V[0]`` holds.  A singular ``V[l][f_ind, :]`` (an exactly
        zero pivot; always when ``f_ind`` repeats a channel) raises ``numpy.linalg.LinAlgError`` naming the first such l."""
        torch = _torch()
        L, F, k = self._stack3(V, "V")
        if not k <= min(self.EIG_TOP_MAX_K, F):
            raise ValueError("constrained_weights: k must be in 1 .. min(%d, F = %d) (got %d)" % (self.EIG_TOP_MAX_K, F, k))
        f_ind = np.asarray(f_ind)
        if f_ind.shape != (k,) or f_ind.dtype.kind not in "iu":
            raise ValueError("f_ind must hold %d integer channel indices (got %r)" % (k, f_ind))
        if f_ind.min() < 0 or f_ind.max() >= F:
            raise ValueError("f_ind must lie in 0 .. %d (got %r)" % (F - 1, f_ind.tolist()))
        fi = np.ascontiguousarray(f_ind, dtype=np.int32)
        W = self.empty((L, F, k))
        info = torch.empty((L,), dtype=torch.int32, device=self.device)
        _check(self.lib.corahip_constrained_weights(self.h, self._f64(V), L, F, k, fi.ctypes.data_as(c_void_p), self._f64(W),
                                                    self._p(info)))
        bad = torch.nonzero(info == 2)
        if bad.numel():
            raise np.linalg.LinAlgError("constrained_weights: the constrained rows of the eigenvectors are singular at l = %d"
                                        % int(bad[0, 0]))
        return W

    def alm_mix_l(self, alm, lmax, W, out=None):
        """``out[f, lm] = sum_j W[l, f, j] alm[j, lm]`` for a_lm in the device layout: ``alm`` [nalm, ceil(k / 4), 2, 4],
        ``W`` [lmax + 1, F, k] on the device, result [nalm, ceil(F / 4), 2, 4].  j is summed in ascending order; the padding
        channels of ``alm`` are not used and those of the result are zero.  ``out`` must not overlap an input."""
        torch = _torch()
        lmax = int(lmax)
        nalm = (lmax + 1) * (lmax + 2) // 2
        if (not isinstance(alm, torch.Tensor) or alm.dim() != 4 or alm.shape[0] != nalm or tuple(alm.shape[2:]) != (2, 4)
                or alm.dtype != torch.float64 or alm.device != self.device or not alm.is_contiguous() or alm.shape[1] < 1):
            raise ValueError("alm must be a contiguous float64 [%d, G, 2, 4] tensor on %s" % (nalm, self.device))
        G = int(alm.shape[1])
        L, F, k = self._stack3(W, "W")
        if L != lmax + 1 or not 4 * (G - 1) < k <= 4 * G:
            raise ValueError("W must be [lmax + 1, F, k] with %d < k <= %d (got %r)" % (4 * (G - 1), 4 * G, tuple(W.shape)))
        out = self._out_like(out, (nalm, (F + 3) // 4, 2, 4), "alm_mix_l")
        for t, name in ((alm, "alm"), (W, "W")):
            if self._overlap(out, out.numel() * 8, t, t.numel() * 8):
                raise ValueError("alm_mix_l: out overlaps %s" % name)
        if out.data_ptr() % 32 or alm.data_ptr() % 32:
            raise ValueError("alm_mix_l: alm and out must be 32-byte aligned")
        _check(self.lib.corahip_alm_mix_l(self.h, self._f64(alm), lmax, k, self._f64(W), F, self._f64(out)))
        return out

    def sht_rings(self, nside, lmax):
        plan = self.sht_plan(nside, lmax)
        nring = 4 * nside - 1
        start = np.zeros(nring, dtype=np.int64)
        nphi = np.zeros(nring, dtype=np.int32)
        z = np.zeros(nring)
        phi0 = np.zeros(nring)
        _check(self.lib.corahip_sht_plan_rings(plan, start.ctypes.data_as(c_void_p), nphi.ctypes.data_as(c_void_p),
                                               z.ctypes.data_as(c_void_p), phi0.ctypes.data_as(c_void_p)))
        return dict(start=start, nphi=nphi, z=z, phi0=phi0)

    def sht_ring_classes(self, nside, lmax):
        """Ring-FFT class of every ring as the synthesis kernels take it: 0 = direct transform, else the Bluestein
        length (a power of two or 3 * 2^k)."""
        cls = np.zeros(4 * nside - 1, dtype=np.int32)
        _check(self.lib.corahip_sht_plan_ring_classes(self.sht_plan(nside, lmax), cls.ctypes.data_as(c_void_p)))
        return cls

    def sht_lambda(self, nside, lmax, m, ring_pair):
        plan = self.sht_plan(nside, lmax)
        out = self.empty((lmax - m + 1,))
        _check(self.lib.corahip_sht_lambda(self.h, plan, m, ring_pair, self._f64(out)))
        return out

    def sht_lambda_entry(self, nside, lmax, m, ring_pair, kq):
        """lambda_lm as lane group ``kq`` of the synthesis kernel forms them (entry at a window start from the plan's
        four entry states per (m, ring))."""
        plan = self.sht_plan(nside, lmax)
        out = self.empty((lmax - m + 1,))
        _check(self.lib.corahip_sht_lambda_entry(self.h, plan, m, ring_pair, kq, self._f64(out)))
        return out

    def sht_lambda_segment_entry(self, nside, lmax, rt, m, ring_pair, kq):
        """lambda_lm as lane group ``kq`` of the scalar synthesis kernel forms them for ring tiles of ``128 rt`` ring
        pairs (``rt`` = 1: 64 and more channels per call, 2: fewer): zero outside the rows the group feeds.  Returns
        ``(lambda [lmax - m + 1], (l_begin, T, R_kq, entry row or -1))``."""
        torch = _torch()
        plan = self.sht_plan(nside, lmax)
        out = self.empty((lmax - m + 1,))
        info = self.empty((4,), dtype=torch.int32)
        _check(self.lib.corahip_sht_lambda_segment_entry(self.h, plan, rt, m, ring_pair, kq, self._f64(out), self._p(info)))
        return out, tuple(int(v) for v in info.cpu().tolist())

    def debug_poison_scratch(self, byte):
        """Test hook (``corahip_debug_poison_scratch``): fills every scratch slot the library holds on this context with
        ``byte`` (0 .. 255), marks its caches in those slots invalid and has later scratch growth and the per-call
        allocations of the eigen routes filled with it; ``byte < 0`` ends that.  Returns the bytes of each slot at the
        call.  CoraHipError (status CORAHIP_ESTATE) while a draw session is pending."""
        sizes = (c_size_t * DEBUG_NSCRATCH)()
        _check(self.lib.corahip_debug_poison_scratch(self.h, int(byte), sizes))
        return [int(v) for v in sizes]


_contexts = {}


def get_context(device=None):
    """Cached Context for `device` (default: torch's current CUDA device)."""
    torch = _torch()
    if device is None:
        device = torch.cuda.current_device() if torch.cuda.is_available() else 0
    if device not in _contexts:
        _contexts[device] = Context(device)
    ctx = _contexts[device]
    ctx.use_current_stream()
    return ctx
