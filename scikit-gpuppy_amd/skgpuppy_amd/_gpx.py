"""ctypes binding of libgpx (include/gpx.h) -- the thin C-ABI under the skgpuppy-compatible classes.

There is no CPU fallback: if libgpx.so is missing the import fails, and if no gfx950 device is visible
every compute call raises.  Status codes follow include/gpx.h: >0 LAPACK-style info ->
numpy.linalg.LinAlgError (what the reference surfaces, skgpuppy/Covariance.py:213,309), GPX_ERR_BAD_ARG
-> ValueError, anything else -> RuntimeError with gpx_last_error().
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("GPX_LIB", os.path.join(_HERE, "libgpx.so"))   # GPX_LIB: diagnostic builds only

GPX_ERR_BAD_ARG, GPX_ERR_HIP, GPX_ERR_NO_DEVICE, GPX_ERR_STATE = -1, -2, -3, -4
K_GRAM, K_GEMM, K_POTRF_LEAF, K_TRSV, K_REDUCE, K_QUAD, K_EXACT, K_GEMM_SMALL, K_TRSV_RIDE, K_GEMM_EMU = range(10)
KERNEL_CLASS_NAMES = ["gram", "gemm_f64_mfma", "potrf_leaf", "trsv", "predict_reduce", "approx_quad", "exact_sum",
                      "gemm_f64_mfma_small_tiles", "trsv_under_factorisation", "gemm_f64_emulated_int8"]

# GPX_GEMM_TRI_* and GPX_GEMM_V_* of include/gpx.h (gpx_dev_gemm_nt_ex; tests/test_gemm_exact_helpers.py holds the two copies together)
ROWS_APPROX, ROWS_DVH, ROWS_GRAD, ROWS_SKIP_NULLABLE = 0, 1, 2, 0x100     # GPX_ROWS_* of include/gpx.h (gpx_rows_build, gpx_rows_reduce)
GEMM_TRI_NONE, GEMM_TRI_A_UPPER, GEMM_TRI_A_LOWER, GEMM_TRI_B_LOWER, GEMM_TRI_B_UPPER = 0, 1, 2, 3, 5


def gemm_variant(wm, wn, lower, form):
    return wm | (wn << 4) | (lower << 8) | (form << 12)


GEMM_VARIANTS = {
    "NONE": 0,
    "128X128": gemm_variant(4, 4, 0, 0), "64X64": gemm_variant(2, 2, 0, 0), "64X128": gemm_variant(2, 4, 0, 0), "32X128": gemm_variant(1, 4, 0, 0),
    "LOWER_128X128": gemm_variant(4, 4, 1, 0), "LOWER_64X64": gemm_variant(2, 2, 1, 0), "LOWER_32X32": gemm_variant(1, 1, 1, 0),
    "TRIB_FINE": gemm_variant(2, 2, 0, 1), "TRIB_LONGEST_FIRST": gemm_variant(4, 4, 0, 2), "TRIB_PAIRED": gemm_variant(4, 4, 0, 3),
    "TRIB_SMALL_64X64": gemm_variant(2, 2, 0, 4), "TRIB_SMALL_64X128": gemm_variant(2, 4, 0, 4), "TRIB_SMALL_32X128": gemm_variant(1, 4, 0, 4),
}

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libgpx.so not found at %s: build it with `make -C scikit-gpuppy_amd/csrc` (or "
        "`python -c 'import __graft_entry__ as g; g.build()'`). There is no CPU fallback." % LIB_PATH)

lib = ctypes.CDLL(LIB_PATH)

_dp = ctypes.c_void_p          # double* that may be a host or a device pointer
_i64 = ctypes.c_int64
_int = ctypes.c_int
_dbl = ctypes.c_double
_hp = ctypes.c_void_p          # gpx_handle*

# name -> (restype, argtypes): every symbol include/gpx.h declares
SIGNATURES = {
    "gpx_abi_version": (_int, []),
    "gpx_last_error": (ctypes.c_char_p, []),
    "gpx_device_count": (_int, []),
    "gpx_set_device": (_int, [_int]),
    "gpx_pool_trim": (_int, []),
    "gpx_gram": (_int, [_dp, _i64, _dp, _i64, _int, _dp, _dbl, _dp]),
    "gpx_fit": (_int, [_dp, _dp, _i64, _int, _dp, ctypes.c_void_p, ctypes.POINTER(_hp)]),
    "gpx_fit_matrix": (_int, [_dp, _dp, _i64, ctypes.c_void_p, ctypes.POINTER(_hp)]),
    "gpx_predict_kv": (_int, [_hp, _dp, _i64, _dp, _dp, _dp]),
    "gpx_nll_grad_matrix": (_int, [_hp, _dp, ctypes.POINTER(_dbl)]),
    "gpx_symv": (_int, [_dp, _i64, _dp, _int, _dp]),
    "gpx_free": (None, [_hp]),
    "gpx_n": (_int, [_hp, ctypes.POINTER(_i64), ctypes.POINTER(_int)]),
    "gpx_jitter_used": (_int, [_hp, ctypes.POINTER(_dbl)]),
    "gpx_logdet": (_int, [_hp, ctypes.POINTER(_dbl)]),
    "gpx_spd_inverse": (_int, [_dp, _i64, _dp, ctypes.POINTER(_dbl)]),
    "gpx_predict": (_int, [_hp, _dp, _i64, _dp, _dp]),
    "gpx_predict_mean_grad": (_int, [_hp, _dp, _i64, _dp, _dp]),
    "gpx_predict_grad": (_int, [_hp, _dp, _i64, _dp, _dp, _dp, _dp]),
    "gpx_alpha": (_int, [_hp, _dp]),
    "gpx_solve": (_int, [_hp, _dp, _int, _dp, _dp]),
    "gpx_chol_mul": (_int, [_hp, _dp, _int, _dp]),
    "gpx_kinv": (_int, [_hp, _dp]),
    "gpx_chol": (_int, [_hp, _dp]),
    "gpx_chol_rows": (_int, [_hp, _i64, _i64, _dp]),
    "gpx_kinv_rows": (_int, [_hp, _i64, _i64, _dp]),
    "gpx_cjh": (_int, [_hp, _dp, _dp, _dp, _dp]),
    "gpx_propagate_approx": (_int, [_hp, _dp, _dp] + [ctypes.POINTER(_dbl)] * 4),
    "gpx_propagate_approx_many": (_int, [_hp, _dp, _dp, _int, _i64, _dp, _dp, _dp, _dp]),
    "gpx_propagate_approx_rows": (_int, [_hp, _dp, _dp, _i64, _i64, _dp]),
    "gpx_propagate_approx_rhs": (_int, [_hp, _dp, _dp, _int, _int, _dp]),
    "gpx_propagate_dvh": (_int, [_hp, _dp, _dp]),
    "gpx_propagate_dvh_many": (_int, [_hp, _dp, _i64, _dp, _dp]),
    "gpx_propagate_quadrature_many": (_int, [_hp, _dp, _dp, _int, _i64, _dp, _dp, _i64, _dp, _i64, _int, _dbl, _dp, _dp]),
    "gpx_mixture_reduce": (_int, [_dp, _dp, _dp, _i64, _i64, _dp, _i64, _int, _dbl, _dp, _dp]),
    "gpx_quadrature_nodes": (_int, [_dp, _dp, _int, _i64, _dp, _i64, _int, _dp]),
    "gpx_propagate_exact": (_int, [_hp, _dp, _dp, ctypes.POINTER(_dbl), ctypes.POINTER(_dbl)]),
    "gpx_propagate_exact_many": (_int, [_hp, _dp, _dp, _int, _i64, _dp, _dp]),
    "gpx_propagate_exact_grad_many": (_int, [_hp, _dp, _dp, _int, _i64, _dp, _dp, _dp, _dp, _dp, _dp]),
    "gpx_propagate_exact_rows": (_int, [_hp, _dp, _dp, _i64, _i64, _dp]),
    "gpx_exact_mean": (_int, [_hp, _dp, _dp, ctypes.POINTER(_dbl)]),
    "gpx_propagate_exact_matrix": (_int, [_hp, _dp, _dp, _dp, _i64, _int, _dp, _dp, _dp, _dp, _dbl, ctypes.POINTER(_dbl), ctypes.POINTER(_dbl)]),
    "gpx_kinv_model_create": (_int, [_dp, _dp, _i64, ctypes.POINTER(_hp)]),
    "gpx_kinv_model_free": (None, [_hp]),
    "gpx_propagate_exact_model": (_int, [_hp, _dp, _int, _dp, _dp, _dp, _dp, _dbl, ctypes.POINTER(_dbl), ctypes.POINTER(_dbl)]),
    "gpx_sensitivity_many": (_int, [_hp, _dp, _dp, _int, _i64, _dp, _dp, _dp, _dp]),
    "gpx_nll": (_int, [_hp, ctypes.POINTER(_dbl)]),
    "gpx_nll_grad": (_int, [_hp, _dp]),
    "gpx_periodic_gram": (_int, [_dp, _i64, _dp, _i64, _int, _dp, _int, _dp]),
    "gpx_periodic_fit": (_int, [_dp, _dp, _i64, _int, _dp, ctypes.c_void_p, ctypes.POINTER(_hp)]),
    "gpx_periodic_predict": (_int, [_hp, _dp, _i64, _dp, _dp]),
    "gpx_periodic_nll_grad": (_int, [_hp, _dp]),
    "gpx_matern_gram": (_int, [_dp, _i64, _dp, _i64, _int, _dp, _int, _int, _dp]),
    "gpx_matern_fit": (_int, [_dp, _dp, _i64, _int, _dp, _int, ctypes.c_void_p, ctypes.POINTER(_hp)]),
    "gpx_matern_predict": (_int, [_hp, _dp, _i64, _dp, _dp]),
    "gpx_matern_nll_grad": (_int, [_hp, _dp]),
    "gpx_matern_propagate_approx_many": (_int, [_hp, _dp, _dp, _int, _i64, _dp, _dp, _dp, _dp]),
    "gpx_matern_propagate_dvh_many": (_int, [_hp, _dp, _i64, _dp, _dp]),
    "gpx_rows_build": (_int, [_hp, _int, _dp, _dp, _int, _i64, _dp]),
    "gpx_rows_reduce": (_int, [_int, _int, _i64, _dp, _dp, _dp, _int, _i64, _dbl, _dp]),
    "gpx_spgp_fit": (_int, [_dp, _dp, _i64, _int, _dp, _dp, _i64, ctypes.POINTER(_hp)]),
    "gpx_spgp_free": (None, [_hp]),
    "gpx_spgp_predict": (_int, [_hp, _dp, _i64, _dp, _dp]),
    "gpx_spgp_nll": (_int, [_hp, ctypes.POINTER(_dbl)]),
    "gpx_spgp_nll_grad": (_int, [_hp, _dp]),
    "gpx_spgp_dense": (_int, [_hp, _int, _dp]),
    "gpx_spgp_cross": (_int, [_hp, _dp, _i64, _dp, _i64, _dp]),
    "gpx_spgp_split": (_int, [_hp, ctypes.POINTER(_int)]),
    "gpx_spgp_pseudo_handle": (_int, [_hp, ctypes.POINTER(_hp)]),
    "gpx_profile_enable": (_int, [_hp, _int]),
    "gpx_profile_reset": (_int, [_hp]),
    "gpx_profile_read": (_int, [_hp, _int, ctypes.POINTER(_i64), ctypes.POINTER(_dbl), ctypes.POINTER(_dbl)]),
    "gpx_bench_mfma_f64": (_int, [_int, ctypes.POINTER(_dbl)]),
    "gpx_bench_emu_i8": (_int, [_i64, _i64, _i64, _int, _int, ctypes.POINTER(_dbl)]),
    "gpx_emu_gemm_nt_sub": (_int, [_dp, _i64, _dp, _i64, _dp, _i64, _i64, _i64, _i64]),
    "gpx_emu_syrk_lower_sub": (_int, [_dp, _i64, _i64, _i64, _dp, _i64, _i64]),
    "gpx_emu_syrk_lower_sub_ex": (_int, [_dp, _i64, _i64, _i64, _dp, _i64, _i64, _int, _i64]),
    "gpx_emu_rebuild": (_int, [_dp, _i64, _i64, _int, _dp, _dp, _dp, _i64, _i64, _i64]),
    "gpx_emu_rebuild_ex": (_int, [_dp, _i64, _i64, _int, _dp, _dp, _dp, _i64, _i64, _i64, _i64, _i64]),
    "gpx_emu_i8_gemm": (_int, [_dp, _dp, _i64, _i64, _i64, _int, _dp]),
    "gpx_emu_i8_gemm_ld": (_int, [_dp, _i64, _dp, _i64, _i64, _i64, _int, _dp, _i64]),
    "gpx_emu_split": (_int, [_dp, _i64, _i64, _i64, _i64, _int, _int, _dp, _i64, _dp]),
    "gpx_emu_split_fixed": (_int, [_dp, _i64, _i64, _i64, _i64, _int, _int, _dp, _i64, _i64, _dp, _dp]),
    "gpx_emu_trsm_left": (_int, [_hp, _dp, _i64, _i64, _dp, _dp, _i64, ctypes.POINTER(_int)]),
    "gpx_bench_hbm": (_int, [_i64, _int, ctypes.POINTER(_dbl), ctypes.POINTER(_dbl)]),
    "gpx_bench_fp64_pipes": (_int, [_int, _int, _int] + [ctypes.POINTER(_dbl)] * 3),
    "gpx_dev_gram": (_int, [_dp, _i64, _dp, _i64, _int, _dp, _dbl, _int, _int, _dp, _i64, _i64, _i64, ctypes.c_void_p]),
    "gpx_dev_gram_scaled": (_int, [_dp, _i64, _dp, _i64, _int, _dbl, _dbl, _int, _int, _dp, _i64, _i64, _i64, ctypes.c_void_p]),
    "gpx_dev_gemm_nt": (_int, [_dp, _i64, _dp, _i64, _dp, _i64, _i64, _i64, _i64, _dbl, _dbl, _int, ctypes.c_void_p]),
    "gpx_dev_gemm_nt_ex": (_int, [_dp, _i64, _dp, _i64, _dp, _i64, _i64, _i64, _i64, _dbl, _dbl, _int, _int, _int, _int, ctypes.POINTER(_int),
                                  ctypes.c_void_p]),
    "gpx_dev_gemm_nt_tri_reduce": (_int, [_dp, _i64, _dp, _i64, _dp, _i64, _i64, _i64, _dbl, _dp, _dp, _dp, _i64, _i64, ctypes.c_void_p]),
    "gpx_dev_gemm_nt_batched": (_int, [_dp, _i64, _i64, _i64, _dp, _i64, _i64, _i64, _dp, _i64, _i64, _i64, _int, _int, _i64, _i64, _i64, _dbl,
                                       _dbl, _i64, ctypes.c_void_p]),
    "gpx_dev_syrk_splitk": (_int, [_dp, _i64, _dp, _dp, _i64, _i64, _int, _dbl, ctypes.c_void_p]),
    "gpx_dev_syrk_trap": (_int, [_dp, _i64, _dp, _i64, _dp, _i64, _i64, _i64, _i64, _dbl, _dbl, ctypes.c_void_p, ctypes.c_void_p]),
    "gpx_dev_syrk_trap_cols": (_int, [_dp, _i64, _dp, _i64, _dp, _i64, _i64, _i64, _i64, _dbl, _dbl, _i64, ctypes.c_void_p, ctypes.c_void_p]),
    "gpx_dev_potrf_leaf": (_int, [_dp, _i64, _dp, _dp, ctypes.c_void_p, _int, ctypes.c_void_p]),
    "gpx_dev_chol_panel": (_int, [_dp, _i64, _i64, _i64, _i64, _dp, _dp, ctypes.c_void_p, ctypes.c_void_p]),
    "gpx_dev_chol_panel_next": (_int, [_dp, _i64, _i64, _i64, _i64, _dp, _i64, _i64, _dp, _dp, ctypes.c_void_p, ctypes.c_void_p]),
    "gpx_dev_chol_panel_split": (_int, [_dp, _i64, _i64, _i64, _i64, _i64, _dp, _i64, _i64, _dp, _dp, ctypes.c_void_p, ctypes.c_void_p,
                                        ctypes.c_void_p, ctypes.c_void_p]),
    "gpx_dev_set_panel_share": (_int, [_int]),
    "gpx_dev_chol_dataflow": (_int, [_dp, _i64, _i64, _i64, _dp, _dp, ctypes.c_void_p, ctypes.c_void_p]),
    "gpx_adopt_factor": (_int, [_dp, _dp, _i64, _int, _dp, _dp, _dp, _dp, _dbl, ctypes.c_void_p, ctypes.POINTER(_hp)]),
    "gpx_multi_fit": (_int, [_dp, _dp, _i64, _int, _dp, ctypes.POINTER(_int), _int, ctypes.POINTER(_hp)]),
    "gpx_multi_free": (None, [_hp]),
    "gpx_multi_info": (_int, [_hp, ctypes.POINTER(_int), ctypes.POINTER(_i64), ctypes.POINTER(_dbl)]),
    "gpx_multi_alpha": (_int, [_hp, _dp]),
    "gpx_multi_predict": (_int, [_hp, _dp, _i64, _dp, _dp]),
    "gpx_multi_propagate_approx": (_int, [_hp, _dp, _dp] + [ctypes.POINTER(_dbl)] * 4),
    "gpx_multi_propagate_exact": (_int, [_hp, _dp, _dp] + [ctypes.POINTER(_dbl)] * 2),
}
for _name, (_res, _args) in SIGNATURES.items():
    try:
        _f = getattr(lib, _name)      # AttributeError here = header and library out of sync
    except AttributeError:
        if "GPX_LIB" in os.environ:   # a diagnostic build of another round (A/B on one box): its missing entry points fail when called
            continue
        raise
    _f.restype = _res
    _f.argtypes = _args


def last_error():
    msg = lib.gpx_last_error()
    return msg.decode("utf-8", "replace") if msg else ""


def check(status, what):
    if status == 0:
        return
    msg = "%s failed (status %d): %s" % (what, status, last_error())
    if status > 0:
        raise np.linalg.LinAlgError(msg)
    if status == GPX_ERR_BAD_ARG:
        raise ValueError(msg)
    raise RuntimeError(msg)


def f64(a):
    """C-contiguous float64 view/copy of array-like `a` (the reference accepts int arrays and lists)."""
    return np.ascontiguousarray(a, dtype=np.float64)


def ptr(a):
    """void* of a NumPy array (host) -- keep `a` alive for the duration of the call."""
    return ctypes.c_void_p(a.ctypes.data)


def device_count():
    return int(lib.gpx_device_count())
