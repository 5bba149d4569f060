"""ctypes binding of libkdehip.so (the C ABI declared in include/kdehip.h).

There is no Python/CPU fallback: if the shared library is missing this module raises at import, and
every compute entry point fails with KDEHIP_ERR_NO_DEVICE when no MI355X is usable.
"""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("KDEHIP_LIB", os.path.join(_HERE, "libkdehip.so"))  # KDEHIP_LIB: diagnostic builds

f64p = C.POINTER(C.c_double)
i64p = C.POINTER(C.c_int64)
i32p = C.POINTER(C.c_int32)
u8p = C.POINTER(C.c_uint8)

KDEHIP_OK = 0
ERR_ARG, ERR_DIM_MISMATCH, ERR_RAND_SHORT, ERR_NO_DEVICE, ERR_HIP, ERR_ALLOC, ERR_UNSUPPORTED = -1, -2, -3, -4, -5, -6, -7
MAX_DIMS, MAX_DENS = 8, 16


class CDensity(C.Structure):
    """struct kdehip_density"""
    _fields_ = [
        ("npts", C.c_int64), ("ndim", C.c_int64),
        ("means", f64p), ("bandwidth", f64p), ("weights", f64p),
        ("left_child", i64p), ("right_child", i64p), ("permutation", i64p),
    ]


class CBatchItem(C.Structure):
    """struct kdehip_batch_item"""
    _fields_ = [
        ("Ndens", C.c_int32), ("Niter", C.c_int32), ("trees", C.POINTER(C.c_void_p)), ("Np", C.c_int64),
        ("seed", C.c_uint64), ("sample_offset", C.c_int64), ("addEntropy", C.c_int32), ("reserved_", C.c_int32),
        ("partialDimMask", u8p), ("d_points", C.c_void_p), ("d_indices", C.c_void_p), ("d_labels", C.c_void_p),
    ]


class CMulItem(C.Structure):
    """struct kdehip_mul_item"""
    _fields_ = [("Ndens", C.c_int32), ("addEntropy", C.c_int32), ("trees", C.POINTER(C.c_void_p)), ("seed", C.c_uint64)]


class CSampleItem(C.Structure):
    """struct kdehip_sample_item"""
    _fields_ = [("density", C.c_void_p), ("Npts", C.c_int64), ("seed", C.c_uint64), ("sample_offset", C.c_int64),
                ("d_ind_in", C.c_void_p), ("d_pts", C.c_void_p), ("d_ind", C.c_void_p)]


class CSampleManifoldItem(C.Structure):
    """struct kdehip_sample_manifold_item (the item's fields are reachable on the outer struct: no nested access per item)"""
    _anonymous_ = ("item",)
    _fields_ = [("item", CSampleItem), ("circular_mask", C.c_uint32), ("reserved_", C.c_uint32)]


class CLoglItem(C.Structure):
    """struct kdehip_logl_item"""
    _fields_ = [("bd", C.c_void_p), ("at", C.c_void_p), ("leave_one_out", C.c_int32), ("reserved_", C.c_int32)]


class CLoglManifoldItem(C.Structure):
    """struct kdehip_logl_manifold_item"""
    _fields_ = [("bd", C.c_void_p), ("at", C.c_void_p), ("leave_one_out", C.c_int32), ("circular_mask", C.c_uint32)]


class CKsumItem(C.Structure):
    """struct kdehip_ksum_item (`var` is a HOST pointer or NULL)"""
    _fields_ = [("a", C.c_void_p), ("b", C.c_void_p), ("var", f64p), ("circular_mask", C.c_uint32), ("normalize", C.c_int32)]


class CMeanshiftItem(C.Structure):
    """struct kdehip_meanshift_item"""
    _fields_ = [("bd", C.c_void_p), ("d_start", C.c_void_p), ("nstart", C.c_int64), ("d_x", C.c_void_p), ("d_logp", C.c_void_p),
                ("d_iters", C.c_void_p), ("circular_mask", C.c_uint32), ("reserved_", C.c_uint32)]


class CHessItem(C.Structure):
    """struct kdehip_hess_item"""
    _fields_ = [("bd", C.c_void_p), ("d_pos", C.c_void_p), ("Nq", C.c_int64), ("d_logp", C.c_void_p), ("d_grad", C.c_void_p),
                ("d_hess", C.c_void_p), ("d_cov", C.c_void_p), ("d_definite", C.c_void_p), ("circular_mask", C.c_uint32),
                ("reserved_", C.c_uint32)]


class CBoxMassItem(C.Structure):
    """struct kdehip_box_mass_item"""
    _fields_ = [("bd", C.c_void_p), ("d_lo", C.c_void_p), ("d_hi", C.c_void_p), ("Nq", C.c_int64), ("d_mass", C.c_void_p),
                ("dim_mask", C.c_uint64), ("circular_mask", C.c_uint32), ("reserved_", C.c_uint32)]


class CQuantileItem(C.Structure):
    """struct kdehip_quantile_item"""
    _fields_ = [("bd", C.c_void_p), ("d_alpha", C.c_void_p), ("Nq", C.c_int64), ("d_x", C.c_void_p), ("d_resid", C.c_void_p),
                ("d_iters", C.c_void_p), ("d_converged", C.c_void_p), ("dim", C.c_int32), ("circular_mask", C.c_uint32)]


class CConditionalItem(C.Structure):
    """struct kdehip_conditional_item"""
    _fields_ = [("bd", C.c_void_p), ("d_given", C.c_void_p), ("Nq", C.c_int64), ("seed", C.c_uint64), ("sample_offset", C.c_int64),
                ("d_logz", C.c_void_p), ("d_mean", C.c_void_p), ("d_var", C.c_void_p), ("d_pts", C.c_void_p), ("d_ind", C.c_void_p),
                ("given_mask", C.c_uint32), ("circular_mask", C.c_uint32)]


class CProdExactItem(C.Structure):
    """struct kdehip_prod_exact_item"""
    _fields_ = [("p", C.c_void_p), ("q", C.c_void_p), ("Np", C.c_int64), ("seed", C.c_uint64), ("sample_offset", C.c_int64),
                ("d_pts", C.c_void_p), ("d_ind", C.c_void_p), ("d_logz", C.c_void_p)]


class CBwJointItem(C.Structure):
    """struct kdehip_bwjoint_item (`start` and the four results are HOST pointers)"""
    _fields_ = [("bd", C.c_void_p), ("start", f64p), ("bw_out", f64p), ("logl", f64p), ("iters", i32p), ("status", i32p),
                ("circular_mask", C.c_uint32), ("reserved_", C.c_uint32)]


class CSinkhornItem(C.Structure):
    """struct kdehip_sinkhorn_item (`scale` and the five results are HOST pointers, the four vectors DEVICE addresses)"""
    _fields_ = [("p", C.c_void_p), ("q", C.c_void_p), ("scale", f64p), ("scale_p", C.c_void_p), ("scale_q", C.c_void_p), ("reg", C.c_double), ("tol", C.c_double),
                ("value", f64p), ("transport_cost", f64p), ("err", f64p), ("mass", f64p), ("iters", i32p),
                ("d_phi", C.c_void_p), ("d_gamma", C.c_void_p), ("d_delta", C.c_void_p), ("d_map", C.c_void_p),
                ("maxiter", C.c_int32), ("circular_mask", C.c_uint32)]


class CCompressItem(C.Structure):
    """struct kdehip_compress_item (`var`, `ks`, `tree_manifold` and `out` are HOST pointers, the five results DEVICE addresses)"""
    _fields_ = [("p", C.c_void_p), ("var", f64p), ("M", C.c_int64), ("d_idx", C.c_void_p), ("d_points", C.c_void_p),
                ("d_zpick", C.c_void_p), ("d_rpick", C.c_void_p), ("d_self_sum", C.c_void_p), ("flags", C.c_uint32),
                ("circular_mask", C.c_uint32), ("out", C.POINTER(C.c_void_p)), ("ks", f64p), ("tree_manifold", u8p)]


class CRefitItem(C.Structure):
    """struct kdehip_refit_item (`log_evidence` and `ess` are HOST pointers)"""
    _fields_ = [("p", C.c_void_p), ("d_values", C.c_void_p), ("d_delta", C.c_void_p), ("log_evidence", f64p), ("ess", f64p),
                ("kind", C.c_int32), ("leaf_order", C.c_int32), ("circular_mask", C.c_uint32), ("reserved_", C.c_uint32)]


class CSummaryItem(C.Structure):
    """struct kdehip_summary_item"""
    _fields_ = [("density", C.c_void_p), ("extend", C.c_double), ("Ngrid", C.c_int64), ("d_range", C.c_void_p),
                ("d_mean", C.c_void_p), ("d_cov", C.c_void_p), ("d_argmax", C.c_void_p), ("d_values", C.c_void_p)]


class CSummaryManifoldItem(C.Structure):
    """struct kdehip_summary_manifold_item (likewise)"""
    _anonymous_ = ("item",)
    _fields_ = [("item", CSummaryItem), ("circular_mask", C.c_uint32), ("reserved_", C.c_uint32)]


class CProductInfo(C.Structure):
    """struct kdehip_product_info_t"""
    _fields_ = [
        ("ndens", C.c_int32), ("ndims", C.c_int32), ("nlevels", C.c_int32), ("precision", C.c_int32),
        ("nodes_per_sweep", C.c_int64), ("bytes_per_eval", C.c_int64), ("packed_bytes", C.c_int64),
        ("fast_math_path", C.c_int32), ("device", C.c_int32),
    ]


# every symbol include/kdehip.h declares: (restype, argtypes)
SIGNATURES = {
    "kdehip_version": (C.c_int, []),
    "kdehip_last_error": (C.c_char_p, []),
    "kdehip_device_count": (C.c_int, []),
    "kdehip_clear_cache": (None, []),
    "kdehip_gibbs1": (C.c_int, [C.c_int, C.POINTER(CDensity), C.c_int64, C.c_int, f64p, i64p, f64p, C.c_int64,
                                f64p, C.c_int64, C.c_int, C.c_int, u8p, C.c_int]),
    "kdehip_gibbs1_trace": (C.c_int, [C.c_int, C.POINTER(CDensity), C.c_int64, C.c_int, f64p, i64p, f64p, C.c_int64,
                                      f64p, C.c_int64, C.c_int, C.c_int, u8p, C.c_int, i32p]),
    "kdehip_gibbs1_multi": (C.c_int, [C.c_int, C.POINTER(CDensity), C.c_int64, C.c_int, f64p, i64p, f64p, C.c_int64,
                                      f64p, C.c_int64, C.c_int, C.c_int, u8p, C.c_int, C.c_int, i32p]),
    "kdehip_gibbs1_manifold": (C.c_int, [C.c_int, C.POINTER(CDensity), C.c_int64, C.c_int, f64p, i64p, f64p, C.c_int64,
                                         f64p, C.c_int64, C.c_int, C.c_int, u8p, u8p, C.c_int, i32p]),
    "kdehip_prod_philox": (C.c_int, [C.c_int, C.POINTER(CDensity), C.c_int64, C.c_int, f64p, i64p, C.c_uint64, C.c_int,
                                     C.c_int, u8p, C.c_int, C.c_int, C.c_int, i32p]),
    "kdehip_product_multi_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(CDensity), C.c_int, u8p,
                                              C.c_int, C.c_int, C.c_int]),
    "kdehip_product_multi_create_manifold": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(CDensity), C.c_int, u8p,
                                                       u8p, C.c_int, C.c_int, C.c_int]),
    "kdehip_prod_philox_manifold": (C.c_int, [C.c_int, C.POINTER(CDensity), C.c_int64, C.c_int, f64p, i64p, C.c_uint64,
                                              C.c_int, C.c_int, u8p, u8p, C.c_int, C.c_int, C.c_int, i32p]),
    "kdehip_product_multi_destroy": (None, [C.c_void_p]),
    "kdehip_product_multi_ngpus": (C.c_int, [C.c_void_p]),
    "kdehip_product_multi_plan": (C.c_void_p, [C.c_void_p, C.c_int]),
    "kdehip_product_multi_sample_philox": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.c_int64, C.c_int,
                                                     C.POINTER(C.c_void_p), C.POINTER(C.c_void_p),
                                                     C.POINTER(C.c_void_p)]),
    "kdehip_product_multi_transfers_per_product": (C.c_int, [C.c_void_p]),
    "kdehip_product_create": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(CDensity), C.c_int, u8p,
                                        C.c_int, C.c_int]),
    "kdehip_product_create_manifold": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(CDensity), C.c_int, u8p, u8p,
                                                 C.c_int, C.c_int]),
    "kdehip_product_destroy": (None, [C.c_void_p]),
    "kdehip_product_info": (C.c_int, [C.c_void_p, C.POINTER(CProductInfo)]),
    "kdehip_product_randu_per_sample": (C.c_int64, [C.c_void_p, C.c_int]),
    "kdehip_product_randn_per_sample": (C.c_int64, [C.c_void_p]),
    "kdehip_product_fallback_count": (C.c_int64, [C.c_void_p]),
    "kdehip_product_sample_streams": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64,
                                                C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p]),
    "kdehip_product_sample_philox": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.c_int64, C.c_int,
                                               C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kdehip_product_sample_philox_host": (C.c_int, [C.c_void_p, C.c_int64, C.c_int, C.c_uint64, C.c_int64,
                                                    C.c_int, f64p, i64p, i32p]),
    "kdehip_product_screen_stats": (C.c_int, [C.c_void_p, i32p, i64p, i64p]),
    "kdehip_product_set_variant": (C.c_int, [C.c_void_p, C.c_int]),
    "kdehip_product_launch_geometry": (C.c_int, [C.c_void_p, C.c_int64, i32p, i32p]),
    "kdehip_product_kernel_name": (C.c_char_p, [C.c_void_p, C.c_int64]),
    "kdehip_density_upload": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(CDensity), C.c_int]),
    "kdehip_density_free": (None, [C.c_void_p]),
    "kdehip_density_npts": (C.c_int64, [C.c_void_p]),
    "kdehip_density_ndim": (C.c_int, [C.c_void_p]),
    "kdehip_prod_philox_device": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.c_int64, C.c_int, C.c_uint64, C.c_int64,
                                            C.c_int, u8p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kdehip_prod_philox_resident": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.c_int64, C.c_int, C.c_uint64, C.c_int, u8p,
                                              C.c_int, f64p, i64p]),
    "kdehip_philox_fill_uniform": (None, [C.c_uint64, C.c_int64, C.c_int64, C.c_int64, f64p]),
    "kdehip_philox_fill_normal": (None, [C.c_uint64, C.c_int64, C.c_int64, C.c_int64, f64p]),
    "kdehip_evaluate": (C.c_int, [C.POINTER(CDensity), f64p, C.c_int64, C.c_int, f64p, C.c_int]),
    "kdehip_eval_avg_logl": (C.c_int, [C.POINTER(CDensity), C.POINTER(CDensity), C.c_int, f64p, C.c_int]),
    "kdehip_eval_avg_logl_device_batch": (C.c_int, [C.c_int, C.POINTER(CLoglItem), C.c_void_p, C.c_void_p]),
    "kdehip_eval_avg_logl_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, f64p]),
    "kdehip_evaluate_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p]),
    "kdehip_evaluate_device_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kdehip_evaluate_manifold": (C.c_int, [C.POINTER(CDensity), f64p, C.c_int64, C.c_int, f64p, C.c_int, u8p]),
    "kdehip_evaluate_device_manifold": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, u8p]),
    "kdehip_evaluate_device_at_manifold": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u8p]),
    "kdehip_eval_avg_logl_manifold": (C.c_int, [C.POINTER(CDensity), C.POINTER(CDensity), C.c_int, f64p, C.c_int, u8p]),
    "kdehip_eval_avg_logl_device_manifold": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, f64p, u8p]),
    "kdehip_eval_avg_logl_device_batch_manifold": (C.c_int, [C.c_int, C.POINTER(CLoglManifoldItem), C.c_void_p, C.c_void_p]),
    "kdehip_evaluate_log": (C.c_int, [C.POINTER(CDensity), f64p, C.c_int64, C.c_int, f64p, C.c_int, u8p]),
    "kdehip_evaluate_log_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, u8p]),
    "kdehip_evaluate_log_device_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u8p]),
    "kdehip_eval_avg_logl_log": (C.c_int, [C.POINTER(CDensity), C.POINTER(CDensity), C.c_int, f64p, C.c_int, u8p]),
    "kdehip_eval_avg_logl_log_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, f64p, u8p]),
    "kdehip_eval_avg_logl_log_device_batch": (C.c_int, [C.c_int, C.POINTER(CLoglManifoldItem), C.c_void_p, C.c_void_p]),
    "kdehip_evaluate_tol": (C.c_int, [C.POINTER(CDensity), f64p, C.c_int64, C.c_int, f64p, f64p, f64p, i64p, C.c_int, u8p]),
    "kdehip_evaluate_device_at_tol": (C.c_int, [C.c_void_p, C.c_void_p, f64p, f64p, C.c_void_p, C.c_void_p, C.c_void_p, u8p]),
    "kdehip_knn": (C.c_int, [C.POINTER(CDensity), f64p, C.c_int64, C.c_int, C.c_int, f64p, f64p, i64p, i64p, C.c_int, u8p]),
    "kdehip_knn_device_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, f64p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u8p]),
    "kdehip_kernel_sum": (C.c_int, [C.POINTER(CDensity), C.POINTER(CDensity), f64p, C.c_int, f64p, C.c_int, u8p]),
    "kdehip_kernel_sum_device": (C.c_int, [C.c_void_p, C.c_void_p, f64p, C.c_int, f64p, u8p]),
    "kdehip_kernel_sum_device_batch": (C.c_int, [C.c_int, C.POINTER(CKsumItem), C.c_void_p, C.c_void_p]),
    "kdehip_evaluate_grad": (C.c_int, [C.POINTER(CDensity), f64p, C.c_int64, C.c_int, f64p, f64p, C.c_int, u8p]),
    "kdehip_evaluate_grad_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, u8p, C.c_void_p]),
    "kdehip_meanshift": (C.c_int, [C.POINTER(CDensity), f64p, C.c_int64, f64p, C.c_int, f64p, f64p, i32p, C.c_int, u8p]),
    "kdehip_meanshift_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, f64p, C.c_int, f64p, f64p, i32p, u8p]),
    "kdehip_meanshift_device_batch": (C.c_int, [C.c_int, C.POINTER(CMeanshiftItem), f64p, C.c_int, C.c_void_p]),
    "kdehip_evaluate_hess": (C.c_int, [C.POINTER(CDensity), f64p, C.c_int64, f64p, f64p, f64p, f64p, i32p, C.c_int, u8p]),
    "kdehip_evaluate_hess_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                              C.c_void_p, u8p, C.c_void_p]),
    "kdehip_evaluate_hess_device_batch": (C.c_int, [C.c_int, C.POINTER(CHessItem), C.c_void_p]),
    "kdehip_box_mass": (C.c_int, [C.POINTER(CDensity), C.c_uint64, f64p, f64p, C.c_int64, f64p, C.c_int, u8p]),
    "kdehip_box_mass_device": (C.c_int, [C.c_void_p, C.c_uint64, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, u8p, C.c_void_p]),
    "kdehip_box_mass_device_batch": (C.c_int, [C.c_int, C.POINTER(CBoxMassItem), C.c_void_p]),
    "kdehip_quantile": (C.c_int, [C.POINTER(CDensity), C.c_int, f64p, C.c_int64, f64p, C.c_int, f64p, f64p, i32p, i32p,
                                  C.c_int, u8p]),
    "kdehip_quantile_device": (C.c_int, [C.c_void_p, C.c_int, C.c_void_p, C.c_int64, f64p, C.c_int, C.c_void_p, C.c_void_p,
                                         C.c_void_p, C.c_void_p, u8p, C.c_void_p]),
    "kdehip_quantile_device_batch": (C.c_int, [C.c_int, C.POINTER(CQuantileItem), f64p, C.c_int, C.c_void_p]),
    "kdehip_conditional": (C.c_int, [C.POINTER(CDensity), C.c_uint32, f64p, C.c_int64, C.c_uint64, C.c_int64, f64p, f64p, f64p,
                                     f64p, i64p, C.c_int, u8p]),
    "kdehip_conditional_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_uint64, C.c_int64, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u8p, C.c_void_p]),
    "kdehip_conditional_device_batch": (C.c_int, [C.c_int, C.POINTER(CConditionalItem), C.c_void_p]),
    "kdehip_condition_weights": (C.c_int, [C.POINTER(CDensity), C.c_uint32, f64p, C.c_int64, f64p, f64p, C.c_int, u8p]),
    "kdehip_condition_weights_device": (C.c_int, [C.c_void_p, C.c_uint32, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, u8p,
                                                  C.c_void_p]),
    "kdehip_density_condition_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_uint32, f64p, u8p, u8p]),
    "kdehip_auto_bandwidth_manifold": (C.c_int, [C.c_int64, C.c_int64, f64p, f64p, i32p, C.c_int, u8p]),
    "kdehip_make_density_auto_manifold": (C.c_int, [C.c_int64, C.c_int64, f64p, f64p, i32p, C.c_int, f64p, f64p, f64p, i64p,
                                                    i64p, i64p, i64p, i64p, f64p, f64p, f64p, f64p, u8p]),
    "kdehip_density_from_device_points_manifold": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int64, C.c_int64,
                                                             C.c_int, C.c_void_p, f64p, i32p, u8p]),
    "kdehip_density_marginal_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, i32p]),
    "kdehip_summary_device_batch": (C.c_int, [C.c_int, C.POINTER(CSummaryItem), C.c_void_p]),
    "kdehip_density_summary": (C.c_int, [C.c_void_p, f64p, C.c_int64, f64p, f64p, f64p, f64p, f64p]),
    "kdehip_kde_max": (C.c_int, [C.POINTER(CDensity), C.c_int64, f64p, f64p, C.c_int]),
    "kdehip_inters_intg_appx_is": (C.c_int, [C.POINTER(CDensity), C.POINTER(CDensity), C.c_int64, f64p, C.c_int]),
    "kdehip_inters_intg_appx_is_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, f64p]),
    "kdehip_auto_bandwidth": (C.c_int, [C.c_int64, C.c_int64, f64p, f64p, i32p, C.c_int]),
    "kdehip_make_density_device_supported": (C.c_int, [C.c_int64, C.c_int64]),
    "kdehip_make_densities_device": (C.c_int, [C.c_int, C.c_int64, i64p] + [C.POINTER(C.c_void_p)] * 2 + [C.c_int64] +
                                     [C.POINTER(C.c_void_p)] * 13 + [C.c_int]),
    "kdehip_density_set_bandwidth": (C.c_int, [C.c_int64, C.c_int64, f64p, C.c_int64, f64p, i64p, i64p, f64p, f64p, f64p, f64p]),
    "kdehip_profile_sampler": (None, [C.c_int]),
    "kdehip_profile_phase_read": (C.c_int, [C.c_int, f64p, i64p]),
    "kdehip_selftest_fp32": (C.c_int, [C.c_int, C.c_uint32, C.c_uint64, C.c_int, f64p, C.POINTER(C.c_uint32),
                                      C.POINTER(C.c_uint32)]),
    "kdehip_selftest_exp64": (C.c_int, [C.c_int, C.c_int, C.c_uint64, C.c_uint64, C.c_int, f64p] + [C.POINTER(C.c_uint64)] * 3),
    "kdehip_profile_sampler_read": (C.c_int, [C.c_int, C.c_void_p, f64p, i64p]),
    "kdehip_product_multi_timing": (C.c_int, [C.c_void_p, f64p, f64p]),
    "kdehip_density_from_device_points": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int64, C.c_int64, C.c_int,
                                                    C.c_void_p, f64p, i32p]),
    "kdehip_mul_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_uint64, C.c_int, f64p, i32p]),
    "kdehip_mul_device_batch": (C.c_int, [C.c_int, C.POINTER(CMulItem), C.POINTER(C.c_void_p), f64p, i32p]),
    # the resident entries on a manifold (include/kdehip.h sections 2c-2e): the manifold follows partialDimMask where there is
    # one, and is the last argument of the `*` entries
    "kdehip_prod_philox_device_manifold": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.c_int64, C.c_int, C.c_uint64, C.c_int64,
                                                     C.c_int, u8p, u8p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "kdehip_prod_philox_resident_manifold": (C.c_int, [C.c_int, C.POINTER(C.c_void_p), C.c_int64, C.c_int, C.c_uint64, C.c_int,
                                                       u8p, u8p, C.c_int, f64p, i64p]),
    "kdehip_mul_device_manifold": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_uint64, C.c_int, f64p,
                                             i32p, u8p]),
    "kdehip_mul_device_batch_manifold": (C.c_int, [C.c_int, C.POINTER(CMulItem), u8p, C.POINTER(C.c_void_p), f64p,
                                                   i32p]),
    "kdehip_density_download": (C.c_int, [C.c_void_p, f64p, f64p, f64p, i64p, i64p, i64p, i64p, i64p, f64p, f64p, f64p,
                                          f64p, f64p]),
    "kdehip_prod_philox_batch": (C.c_int, [C.c_int, C.POINTER(CBatchItem), C.c_int, C.c_void_p]),
    "kdehip_prod_philox_batch_manifold": (C.c_int, [C.c_int, C.POINTER(CBatchItem), u8p, C.c_int, C.c_void_p]),
    "kdehip_prod_philox_batch_launches": (None, [C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "kdehip_sample": (C.c_int, [C.POINTER(CDensity), C.c_int64, C.c_uint64, C.c_int64, i64p, f64p, i64p, C.c_int]),
    "kdehip_sample_device": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p,
                                       C.c_void_p]),
    "kdehip_sample_device_batch": (C.c_int, [C.c_int, C.POINTER(CSampleItem), C.c_void_p]),
    "kdehip_resample_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int64, C.c_uint64, f64p, i32p]),
    "kdehip_make_density_auto": (C.c_int, [C.c_int64, C.c_int64, f64p, f64p, i32p, C.c_int, f64p, f64p, f64p, i64p, i64p, i64p,
                                           i64p, i64p, f64p, f64p, f64p, f64p]),
    "kdehip_make_density": (C.c_int, [C.c_int64, C.c_int64, f64p, f64p, C.c_int64, f64p, f64p, f64p, f64p,
                                      i64p, i64p, i64p, i64p, i64p, f64p, f64p, f64p, f64p]),
    # tree construction on a manifold (include/kdehip.h section 4): the named entry plus a trailing tree_manifold
    "kdehip_make_density_tree": (C.c_int, [C.c_int64, C.c_int64, f64p, f64p, C.c_int64, f64p, f64p, f64p, f64p,
                                           i64p, i64p, i64p, i64p, i64p, f64p, f64p, f64p, f64p, u8p]),
    "kdehip_make_densities_device_tree": (C.c_int, [C.c_int, C.c_int64, i64p] + [C.POINTER(C.c_void_p)] * 2 + [C.c_int64] +
                                          [C.POINTER(C.c_void_p)] * 13 + [C.c_int, u8p]),
    "kdehip_make_density_auto_tree": (C.c_int, [C.c_int64, C.c_int64, f64p, f64p, i32p, C.c_int, f64p, f64p, f64p, i64p,
                                                i64p, i64p, i64p, i64p, f64p, f64p, f64p, f64p, u8p, u8p]),
    "kdehip_density_from_device_points_tree": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int64, C.c_int64,
                                                         C.c_int, C.c_void_p, f64p, i32p, u8p, u8p]),
    "kdehip_mul_device_tree": (C.c_int, [C.POINTER(C.c_void_p), C.c_int, C.POINTER(C.c_void_p), C.c_uint64, C.c_int, f64p,
                                         i32p, u8p, u8p]),
    "kdehip_mul_device_batch_tree": (C.c_int, [C.c_int, C.POINTER(CMulItem), u8p, u8p, C.POINTER(C.c_void_p), f64p, i32p]),
    "kdehip_summary_device_batch_manifold": (C.c_int, [C.c_int, C.POINTER(CSummaryManifoldItem), C.c_void_p]),
    "kdehip_density_summary_manifold": (C.c_int, [C.c_void_p, f64p, C.c_int64, f64p, f64p, f64p, f64p, f64p, u8p]),
    "kdehip_kde_max_manifold": (C.c_int, [C.POINTER(CDensity), C.c_int64, f64p, f64p, C.c_int, u8p]),
    "kdehip_inters_intg_appx_is_manifold": (C.c_int, [C.POINTER(CDensity), C.POINTER(CDensity), C.c_int64, f64p, C.c_int,
                                                      u8p]),
    "kdehip_inters_intg_appx_is_device_manifold": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, f64p, u8p]),
    "kdehip_density_marginal_device_tree": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int, i32p, u8p]),
    # per-point bandwidths (include/kdehip.h sections 4 and 5o): the builder, and evaluation / log-likelihoods of ANY density
    "kdehip_make_density_varbw": (C.c_int, [C.c_int64, C.c_int64, f64p, f64p, f64p, f64p, f64p, f64p,
                                            i64p, i64p, i64p, i64p, i64p, f64p, f64p, f64p, f64p, u8p]),
    "kdehip_evaluate_varbw": (C.c_int, [C.POINTER(CDensity), f64p, C.c_int64, C.c_int, C.c_int, f64p, C.c_int, u8p]),
    "kdehip_eval_avg_logl_varbw": (C.c_int, [C.POINTER(CDensity), C.POINTER(CDensity), C.c_int, C.c_int, f64p, C.c_int, u8p]),
    "kdehip_evaluate_varbw_device_at": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, u8p]),
    "kdehip_evaluate_varbw_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_void_p, C.c_void_p, u8p]),
    "kdehip_eval_avg_logl_varbw_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, u8p]),
    "kdehip_density_uniform_bandwidth": (C.c_int, [C.c_void_p]),
    # the exact product of two densities (include/kdehip.h section 5p)
    "kdehip_prod_exact": (C.c_int, [C.POINTER(CDensity), C.POINTER(CDensity), C.c_int64, C.c_uint64, C.c_int64, f64p, i64p, f64p,
                                    C.c_int]),
    "kdehip_prod_exact_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p,
                                           C.c_void_p, C.c_void_p]),
    "kdehip_prod_exact_device_batch": (C.c_int, [C.c_int, C.POINTER(CProdExactItem), C.c_void_p]),
    "kdehip_product_components": (C.c_int, [C.POINTER(CDensity), C.POINTER(CDensity), f64p, f64p, f64p, C.c_int]),
    "kdehip_product_components_device": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    # joint bandwidth selection (include/kdehip.h section 5q): blocking, host results
    "kdehip_bandwidth_joint": (C.c_int, [C.POINTER(CDensity), f64p, f64p, C.c_int, f64p, f64p, i32p, i32p, f64p, C.c_int, u8p]),
    "kdehip_bandwidth_joint_device": (C.c_int, [C.c_void_p, f64p, f64p, C.c_int, f64p, f64p, i32p, i32p, f64p, u8p]),
    "kdehip_bandwidth_joint_device_batch": (C.c_int, [C.c_int, C.POINTER(CBwJointItem), f64p, C.c_int]),
    # reweighting and moving a density without re-forming its tree (include/kdehip.h section 5r): blocking, no stream
    "kdehip_density_refit": (C.c_int, [C.c_int64, C.c_int64, f64p, f64p, f64p, i64p, i64p, i64p, i64p, i64p, f64p, f64p, f64p,
                                       f64p, C.c_int, f64p, f64p, u8p, f64p, f64p, f64p, i64p, i64p, i64p, i64p, i64p, f64p,
                                       f64p, f64p, f64p]),
    "kdehip_density_refit_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p, u8p,
                                              f64p, f64p]),
    "kdehip_density_refit_device_batch": (C.c_int, [C.c_int, C.POINTER(CRefitItem), C.POINTER(C.c_void_p)]),
    # entropic optimal transport (include/kdehip.h section 5s): blocking, host scalars, no stream
    "kdehip_sinkhorn": (C.c_int, [C.POINTER(CDensity), C.POINTER(CDensity), f64p, f64p, f64p, C.c_int, f64p, f64p,
                                  f64p, f64p, i32p, f64p, f64p, f64p, f64p, C.c_int, u8p]),
    "kdehip_sinkhorn_device": (C.c_int, [C.c_void_p, C.c_void_p, f64p, f64p, f64p, C.c_int, f64p, f64p, f64p, f64p,
                                         i32p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, u8p]),
    "kdehip_sinkhorn_device_batch": (C.c_int, [C.c_int, C.POINTER(CSinkhornItem)]),
    # compression by kernel herding (include/kdehip.h section 5t): blocking, no stream
    "kdehip_compress": (C.c_int, [C.POINTER(CDensity), C.c_int64, f64p, C.c_int, i64p, f64p, f64p, f64p, C.c_int, u8p]),
    "kdehip_compress_device": (C.c_int, [C.c_void_p, C.c_int64, f64p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                         C.c_void_p, u8p]),
    "kdehip_compress_device_batch": (C.c_int, [C.c_int, C.POINTER(CCompressItem)]),
    "kdehip_density_compress_device": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int64, f64p, f64p, u8p, u8p]),
    "kdehip_sample_manifold": (C.c_int, [C.POINTER(CDensity), C.c_int64, C.c_uint64, C.c_int64, i64p, f64p, i64p, C.c_int,
                                         u8p]),
    "kdehip_sample_device_manifold": (C.c_int, [C.c_void_p, C.c_int64, C.c_uint64, C.c_int64, C.c_void_p, C.c_void_p,
                                                C.c_void_p, C.c_void_p, u8p]),
    "kdehip_sample_device_batch_manifold": (C.c_int, [C.c_int, C.POINTER(CSampleManifoldItem), C.c_void_p]),
    "kdehip_resample_device_manifold": (C.c_int, [C.POINTER(C.c_void_p), C.c_void_p, C.c_int64, C.c_uint64, f64p, i32p,
                                                  u8p, u8p]),
}


class KdeHipError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"libkdehip error {code}: {msg}")
        self.code = code


def _share_hip_runtime_with_torch():
    """PyTorch-ROCm wheels bundle their own libamdhip64.so (no SONAME), while libkdehip.so links the
    system one (libamdhip64.so.7).  Two HIP runtimes in one process fight over the device: whichever
    initialises second sees "No HIP GPUs".  Binding libkdehip's hip* symbols to torch's copy (global
    scope, loaded first) keeps ONE runtime whatever the import order.  No torch -> system runtime."""
    if os.environ.get("KDEHIP_NO_TORCH_HIP") == "1":
        return
    try:
        import importlib.util
        spec = importlib.util.find_spec("torch")
        if spec is None or not spec.submodule_search_locations:
            return
        cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
        if os.path.exists(cand):
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
    except Exception:  # noqa: BLE001  (purely a courtesy; the system runtime still works on its own)
        pass


def _load():
    _share_hip_runtime_with_torch()
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "(hipcc --offload-arch=gfx950).  This package has no CPU fallback.")
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the library does not export a declared symbol
        fn.restype = res
        fn.argtypes = args
    return lib


lib = _load()


def check(rc: int):
    if rc != KDEHIP_OK:
        msg = lib.kdehip_last_error().decode("utf-8", "replace")
        if rc == ERR_DIM_MISMATCH:
            raise ValueError(msg)  # Julia: error("kdes must have same dimension")
        if rc == ERR_RAND_SHORT:
            raise IndexError(msg)  # Julia: BoundsError
        raise KdeHipError(rc, msg)


def ptr(a, t):
    return a.ctypes.data_as(t)


def optr(a, t):
    """an optional array argument: NULL for None"""
    return None if a is None else a.ctypes.data_as(t)


def addr(x):
    """a device address (or a stream) for the ABI: a torch tensor, an integer, or None = NULL"""
    if x is None:
        return None
    if hasattr(x, "data_ptr"):
        return C.c_void_p(x.data_ptr())
    return C.c_void_p(int(x))


SEED_MASK = 2 ** 64 - 1   # a seed is the 64 bits the Philox key takes: `int(seed) & SEED_MASK` in a struct field


def u64(seed):
    """... and as a uint64_t argument"""
    return C.c_uint64(int(seed) & SEED_MASK)


def random_seed() -> int:
    """the seed of a call that was given none: 64 bits from the operating system"""
    return int.from_bytes(os.urandom(8), "little")
