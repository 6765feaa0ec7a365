"""ctypes mirror of include/t2fit.h (structs and constants).  Keep in lock-step with the header."""
from __future__ import annotations

import ctypes as C

ABI_VERSION = 5
MAX_TE = 32

OK, E_INVALID, E_HIP, E_BOUNDS = 0, -1, -2, -3

MODEL_GAUSSIAN, MODEL_GAUSSIAN_RICIAN, MODEL_RICIAN = 0, 1, 2
MODELS = {"gaussian": MODEL_GAUSSIAN, "gaussian_rician": MODEL_GAUSSIAN_RICIAN, "rician": MODEL_RICIAN}

SOLVER_LBFGSB, SOLVER_LM, SOLVER_LOGLIN = 0, 1, 2
SOLVERS = {"lbfgsb": SOLVER_LBFGSB, "L-BFGS-B": SOLVER_LBFGSB, "lm": SOLVER_LM, "loglin": SOLVER_LOGLIN}

PREC_F64, PREC_F32 = 0, 1
PRECISIONS = {"f64": PREC_F64, "f32": PREC_F32}

LAYOUT_TE_MAJOR, LAYOUT_VOXEL_MAJOR = 0, 1

ST_MASKED, ST_CONVERGED, ST_NOT_CONV, ST_NONFINITE, ST_INFEASIBLE = 0, 1, 2, 3, 4


class T2FitConfig(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("model", C.c_int32), ("solver", C.c_int32), ("precision", C.c_int32),
        ("n_te", C.c_int32), ("no_prior", C.c_int32), ("norm", C.c_int32), ("maxls", C.c_int32),
        ("maxiter", C.c_int32), ("maxfun", C.c_int32), ("numpy_legacy", C.c_int32), ("reserved1", C.c_int32),
        ("te_ms", C.c_double * MAX_TE),
        ("x0", C.c_double * 3), ("lb", C.c_double * 3), ("ub", C.c_double * 3),
        ("ftol", C.c_double), ("gtol", C.c_double), ("fd_step", C.c_double), ("lm_xtol", C.c_double),
        ("noprior_k_ub", C.c_double), ("noprior_t2_lb", C.c_double), ("noprior_t2_ub", C.c_double),
    ]


class T2FitMaps(C.Structure):
    _fields_ = [
        ("t2", C.c_void_p), ("k", C.c_void_p), ("sigma", C.c_void_p), ("res", C.c_void_p),
        ("r2", C.c_void_p), ("fun", C.c_void_p), ("nit", C.c_void_p), ("status", C.c_void_p),
        ("t2_se", C.c_void_p),
    ]


BOOT_NOISE_RICIAN, BOOT_NOISE_GAUSSIAN = 0, 1
BOOT_NOISES = {"rician": BOOT_NOISE_RICIAN, "gaussian": BOOT_NOISE_GAUSSIAN}
BOOT_PARAMS = {"t2": 0, "k": 1, "sigma": 2}  # index into T2FitBootMaps; the which_params bit is 1 << index
BOOT_MAX_INTERVAL_REPLICAS = 512


class T2FitBootMaps(C.Structure):
    _fields_ = [("mean", C.c_void_p * 3), ("bias", C.c_void_p * 3), ("std", C.c_void_p * 3),
                ("ci_lo", C.c_void_p * 3), ("ci_hi", C.c_void_p * 3), ("n_ok", C.c_void_p)]


class T2FitTvParams(C.Structure):
    _fields_ = [("weight", C.c_double), ("eps", C.c_double), ("max_iter", C.c_int32), ("dims", C.c_int32),
                ("precision", C.c_int32), ("flags", C.c_int32)]


TV_JOINT_MAX_CHAN = 64
MPPCA_MAX_TE, MPPCA_MAX_RADIUS = 16, 4
SEG_MAX_CLASSES, SEG_MAX_CHANNELS, SEG_MAX_RADIUS = 8, 4, 32
DICT_MAX_ATOMS = 65536
UNRING_MIN_N, UNRING_MAX_N, UNRING_MAX_SHIFTS, UNRING_MAX_WINDOW = 8, 512, 32, 8
COMPONENTS_TILE = (4, 8, 64)  # (z, y, x) voxels of the tile a workgroup labels in LDS
EDT_MAX_AXIS = 2048  # voxels per axis of the distance transform
NNLS_MAX_BASIS, NNLS_MAX_FUNC = 64, 8
NNLS_CHUNK, NNLS_MAX_WAVES = 64, 8  # voxels a wave takes at a time; waves of a workgroup at most
NNLS_MASKED, NNLS_OK, NNLS_MAXITER, NNLS_BREAKDOWN, NNLS_NONFINITE = -1, 0, 1, 2, 3
NNLS_RULE_FOUND, NNLS_RULE_EXACT, NNLS_RULE_LOW, NNLS_RULE_HIGH = 0, 1, 2, 3  # the chi^2 rule; -1: masked or non-finite


class T2FitNnlsParams(C.Structure):
    _fields_ = [("tol_rel", C.c_double), ("piv_rel", C.c_double), ("max_iter", C.c_int32), ("max_blocks", C.c_int32)]


class T2FitNnlsChi2Params(C.Structure):
    _fields_ = [("factor", C.c_double), ("mu_first", C.c_double), ("grow", C.c_double), ("exact_rel", C.c_double), ("mu_exact", C.c_double),
                ("n_grow", C.c_int32), ("n_bisect", C.c_int32)]


class T2FitUnringParams(C.Structure):
    _fields_ = [("K", C.c_int32), ("min_w", C.c_int32), ("max_w", C.c_int32), ("flags", C.c_int32)]


class T2FitMppcaParams(C.Structure):
    _fields_ = [("radius", C.c_int32), ("dims", C.c_int32), ("estimator", C.c_int32), ("flags", C.c_int32)]


INTERP_LINEAR, INTERP_NEAREST = 0, 1
INTERPS = {"linear": INTERP_LINEAR, "nearest": INTERP_NEAREST}
RESAMPLE_F32, RESAMPLE_I32 = 0, 1
RESAMPLE_INTEGER_CAST, RECON_CHAIN = 1, 2  # flags bits

MORPH_DILATE, MORPH_ERODE, MORPH_CLOSE, MORPH_OPEN = 0, 1, 2, 3
MORPH_OPS = {"dilate": MORPH_DILATE, "erode": MORPH_ERODE, "close": MORPH_CLOSE, "open": MORPH_OPEN}
MORPH_UNBOUNDED = 1  # flags bit
MORPH_F32, MORPH_I32, MORPH_U8 = 0, 1, 2

SR_PROFILE_BOX, SR_PROFILE_BSPLINE3 = 0, 1
SR_PROFILES = {"box": SR_PROFILE_BOX, "bspline3": SR_PROFILE_BSPLINE3}
SR_MAX_STACKS = 6
SR_SLICE_RECORD_BYTES = 208
SR_ROBUST_MAX_SLICES = 4096


class T2FitSrRobustParams(C.Structure):
    _fields_ = [("slice_threshold", C.c_double), ("huber", C.c_double), ("sigma_floor", C.c_double), ("min_count", C.c_int32),
                ("flags", C.c_int32)]

REGISTER_SUMS = 43
SVR_RECORD_BYTES = 128
REGISTER_MAX_BINS = 64
REGISTER_MI_SUMS = 12

# every symbol include/t2fit.h declares: (name, restype, argtypes)
_P = C.c_void_p
SYMBOLS = [
    ("t2fit_config_default", C.c_int, [C.POINTER(T2FitConfig), C.c_int, C.c_int]),
    ("t2fit_device_count", C.c_int, []),
    ("t2fit_volume_dev", C.c_int, [C.POINTER(T2FitConfig), _P, C.c_int, _P, C.c_int64, C.POINTER(T2FitMaps), _P]),
    ("t2fit_create", C.c_int, [C.c_int, C.POINTER(_P)]),
    ("t2fit_destroy", C.c_int, [_P]),
    ("t2fit_context_volume_host", C.c_int, [_P, C.POINTER(T2FitConfig), _P, C.c_int, _P, C.c_int64, C.POINTER(T2FitMaps)]),
    ("t2fit_volume_host", C.c_int, [C.POINTER(T2FitConfig), _P, C.c_int, _P, C.c_int64, C.POINTER(T2FitMaps), C.c_int]),
    ("t2fit_voxels_host", C.c_int, [C.POINTER(T2FitConfig), _P, C.c_int, C.c_int64, _P, C.c_int64, _P, _P, _P, _P, C.c_int]),
    ("t2fit_voxels_trace_host", C.c_int, [C.POINTER(T2FitConfig), _P, C.c_int, C.c_int64, _P, C.c_int64, _P, _P, _P, _P,
                                          C.c_int, _P, _P, C.c_int]),
    ("t2fit_union_mask_dev", C.c_int, [_P, C.c_int, C.c_int64, _P, _P, _P, _P]),
    ("t2fit_residuals_dev", C.c_int, [C.POINTER(T2FitConfig), _P, C.c_int, _P, C.c_int64, _P, _P, _P, _P, _P]),
    ("t2fit_label_stats_dev", C.c_int, [_P, _P, C.c_int64, C.c_int, _P, _P, _P, _P]),
    ("t2fit_roi_erode_dev", C.c_int, [_P, _P, C.c_int32, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    ("t2fit_roi_stats_dev", C.c_int, [_P, _P, C.c_int64, C.c_int, _P, _P, _P, _P, _P, _P]),
    ("t2fit_boot_background_dev", C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int64, C.POINTER(C.c_double),
                                            C.POINTER(C.c_int64), _P]),
    ("t2fit_boot_synth_dev", C.c_int, [C.POINTER(T2FitConfig), _P, _P, C.c_double, _P, _P, C.c_int64, C.c_int64, C.c_uint64,
                                       C.c_int, C.c_int, _P, _P]),
    ("t2fit_bootstrap_dev", C.c_int, [_P, C.POINTER(T2FitConfig), _P, _P, _P, C.c_double, _P, C.c_int, _P, C.c_int64, C.c_int,
                                      C.c_uint64, C.c_double, C.c_int, C.POINTER(T2FitBootMaps), C.c_int, _P]),
    ("t2fit_tv_params_default", C.c_int, [C.POINTER(T2FitTvParams)]),
    ("t2fit_tv_workspace_bytes", C.c_int, [C.POINTER(T2FitTvParams), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_tv_denoise_dev", C.c_int, [C.POINTER(T2FitTvParams), _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t,
                                       _P, _P, _P]),
    ("t2fit_tv_joint_workspace_bytes", C.c_int, [C.POINTER(T2FitTvParams), C.c_int, C.c_int, C.c_int, C.c_int,
                                                 C.POINTER(C.c_size_t)]),
    ("t2fit_tv_joint_denoise_dev", C.c_int, [C.POINTER(T2FitTvParams), _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t,
                                             _P, _P, _P]),
    ("t2fit_mppca_params_default", C.c_int, [C.POINTER(T2FitMppcaParams)]),
    ("t2fit_mppca_workspace_bytes", C.c_int, [C.POINTER(T2FitMppcaParams), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_mppca_dev", C.c_int, [C.POINTER(T2FitMppcaParams), _P, _P, _P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t,
                                  _P]),
    ("t2fit_seg_workspace_bytes", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_seg_mask_dev", C.c_int, [_P, _P, C.c_int, C.c_int64, _P, _P]),
    ("t2fit_seg_priors_dev", C.c_int, [_P, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.c_int,
                                       C.POINTER(C.c_double), C.c_int, C.POINTER(C.c_double), C.c_int, _P, _P, _P]),
    ("t2fit_seg_normalise_dev", C.c_int, [_P, _P, C.c_int, C.c_int64, C.c_double, _P, _P]),
    ("t2fit_seg_sums_dev", C.c_int, [_P, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    ("t2fit_seg_estep_dev", C.c_int, [_P, _P, _P, _P, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.c_double, C.c_int, C.c_int, C.c_int,
                                      C.c_int, C.c_int, _P, _P]),
    ("t2fit_seg_labels_dev", C.c_int, [_P, _P, C.POINTER(C.c_int32), C.c_int, C.c_int64, _P, _P]),
    ("t2fit_resample_dev", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), _P, C.c_int, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_double, C.c_int, _P]),
    ("t2fit_reconstruct_workspace_bytes", C.c_int, [C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int,
                                                    C.POINTER(C.c_size_t)]),
    ("t2fit_reconstruct_dev", C.c_int, [C.POINTER(_P), C.POINTER(C.c_int32), C.POINTER(C.c_double), C.POINTER(C.c_int32),
                                        C.POINTER(C.c_double), _P, C.c_int, C.c_int, _P, C.c_size_t, _P]),
    ("t2fit_sr_plan_host", C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int32)]),
    ("t2fit_sr_workspace_bytes", C.c_int, [C.c_int, C.POINTER(C.c_int32), C.c_int, C.c_int, C.c_int, C.c_int,
                                           C.POINTER(C.c_size_t)]),
    ("t2fit_sr_forward_dev", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double),
                                       C.POINTER(C.c_int32), C.c_int, C.c_double, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P]),
    ("t2fit_sr_adjoint_dev", C.c_int, [C.c_int, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int32),
                                       C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_double), _P, C.c_double, _P,
                                       C.c_int, C.c_int, C.c_int, C.c_int, _P]),
    ("t2fit_sr_slice_table_bytes", C.c_int, [C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_sr_slice_table_host", C.c_int, [C.c_int, C.POINTER(C.c_double), C.c_int, C.c_double, _P, C.c_size_t]),
    ("t2fit_sr_slice_forward_dev", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, C.c_double, _P, _P, C.c_int, C.c_int,
                                             C.c_int, _P, _P, _P]),
    ("t2fit_sr_slice_adjoint_dev", C.c_int, [C.c_int, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int32),
                                             C.POINTER(C.c_int32), C.POINTER(C.c_double), _P, C.c_double, _P, C.c_int, C.c_int, C.c_int,
                                             C.c_int, _P]),
    ("t2fit_sr_robust_params_default", C.c_int, [C.POINTER(T2FitSrRobustParams)]),
    ("t2fit_sr_robust_workspace_bytes", C.c_int, [C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_sr_robust_dev", C.c_int, [C.c_int, C.POINTER(_P), C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int32), C.c_int,
                                      C.POINTER(T2FitSrRobustParams), _P, _P, _P, _P]),
    ("t2fit_morph_workspace_bytes", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_binary_threshold_dev", C.c_int, [_P, C.c_int, C.c_int64, C.c_double, C.c_double, _P, _P]),
    ("t2fit_binary_morph_dev", C.c_int, [C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int,
                                         _P, C.c_size_t, _P]),
    ("t2fit_fill_holes_dev", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_size_t, C.POINTER(C.c_int32), _P]),
    ("t2fit_seed_labels_dev", C.c_int, [_P, _P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.c_int, _P, C.c_size_t,
                                        _P]),
    ("t2fit_relabel_dev", C.c_int, [_P, C.c_int64, _P, C.c_int, _P, _P]),
    ("t2fit_components_workspace_bytes", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_components_label_dev", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P, C.POINTER(C.c_int32), _P, C.c_size_t,
                                             _P]),
    ("t2fit_components_stats_dev", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    ("t2fit_components_lut_dev", C.c_int, [_P, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int, _P, C.POINTER(C.c_int32), _P]),
    ("t2fit_edt_workspace_bytes", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_edt_dev", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), _P, _P, _P, C.c_size_t, _P]),
    ("t2fit_edt_fill_dev", C.c_int, [_P, _P, _P, C.c_int64, _P, _P]),
    ("t2fit_register_workspace_bytes", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_register_sums_dev", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int,
                                          C.POINTER(C.c_double), _P, _P, C.c_size_t, _P]),
    ("t2fit_shrink_dev", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    ("t2fit_shrink_mask_dev", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P]),
    ("t2fit_register_bin_dev", C.c_int, [_P, C.c_int64, C.c_double, C.c_double, C.c_int, _P, _P]),
    ("t2fit_register_binned_workspace_bytes", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_register_binned_sums_dev", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int,
                                                 C.POINTER(C.c_double), C.c_int, _P, _P, _P, C.c_size_t, _P]),
    ("t2fit_register_sums_lut_dev", C.c_int, [_P, _P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int,
                                              C.POINTER(C.c_double), _P, _P, C.c_size_t, _P]),
    ("t2fit_register_joint_hist_dev", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int,
                                                C.POINTER(C.c_double), C.c_int, C.c_int, C.c_double, C.c_double, _P, _P]),
    ("t2fit_register_mi_workspace_bytes", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_register_mi_gradient_dev", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_double, C.c_double, _P, C.c_int, C.c_int, C.c_int,
                                                 _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), _P, _P, C.c_size_t, _P]),
    ("t2fit_ffd_workspace_bytes", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_ffd_joint_hist_dev", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), _P,
                                           C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _P, _P, C.c_size_t, _P]),
    ("t2fit_ffd_gradient_dev", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_double, C.c_double, _P, C.c_int, C.c_int, C.c_int, _P, _P, C.c_int,
                                         C.c_int, C.c_int, C.POINTER(C.c_double), _P, C.c_int, _P, _P, C.c_size_t, _P]),
    ("t2fit_ffd_warp_dev", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), _P, C.c_int, _P, C.c_int, C.c_int,
                                     C.c_int, C.c_int, C.c_double, _P, C.c_size_t, _P]),
    ("t2fit_ffd_jacobian_dev", C.c_int, [_P, C.c_int, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    ("t2fit_svr_table_bytes", C.c_int, [C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_svr_table_host", C.c_int, [C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_uint8),
                                       C.c_int, C.POINTER(C.c_int32), _P, C.c_size_t]),
    ("t2fit_svr_workspace_bytes", C.c_int, [C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_svr_sums_dev", C.c_int, [C.c_int, C.POINTER(_P), C.POINTER(_P), C.POINTER(C.c_int32), _P, _P, C.c_int, C.c_int, C.c_int, _P,
                                     C.c_int, _P, _P, C.c_size_t, _P]),
    ("t2fit_n4_workspace_bytes", C.c_int, [C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_n4_log_dev", C.c_int, [_P, _P, C.c_int64, _P, _P, _P]),
    ("t2fit_n4_minmax_dev", C.c_int, [_P, _P, C.c_int64, _P, _P, C.c_size_t, _P]),
    ("t2fit_n4_histogram_dev", C.c_int, [_P, _P, C.c_int64, C.c_double, C.c_double, C.c_int, _P, _P]),
    ("t2fit_n4_weights_dev", C.c_int, [_P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, C.c_size_t, _P]),
    ("t2fit_n4_fit_dev", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, C.c_double, C.c_double, C.c_int, C.c_int, _P, _P, _P, _P,
                                   C.c_size_t, _P]),
    ("t2fit_n4_field_dev", C.c_int, [_P, C.c_int, _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P, _P, C.c_size_t, _P]),
    ("t2fit_n4_apply_dev", C.c_int, [_P, _P, C.c_int64, C.c_double, _P, _P]),
    ("t2fit_dict_pack_bytes", C.c_int, [C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_dict_pack_host", C.c_int, [C.c_int, C.c_int, _P, _P, C.c_size_t]),
    ("t2fit_dict_match_dev", C.c_int, [_P, C.c_int, C.c_int64, _P, _P, _P, _P, _P, _P]),
    ("t2fit_unring_params_default", C.c_int, [C.POINTER(T2FitUnringParams)]),
    ("t2fit_unring_tables_bytes", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_unring_tables_host", C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_size_t]),
    ("t2fit_unring_workspace_bytes", C.c_int, [C.POINTER(T2FitUnringParams), C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_unring_split_dev", C.c_int, [_P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.c_size_t, _P]),
    ("t2fit_unring_rows_dev", C.c_int, [C.POINTER(T2FitUnringParams), _P, _P, C.c_int, C.c_int, C.c_int, C.c_int, _P, _P, _P, _P]),
    ("t2fit_unring_dev", C.c_int, [C.POINTER(T2FitUnringParams), _P, _P, C.c_int, C.c_int, C.c_int, _P, _P, _P, C.POINTER(C.c_int64), _P,
                                   C.c_size_t, _P]),
    ("t2fit_nnls_params_default", C.c_int, [C.POINTER(T2FitNnlsParams)]),
    ("t2fit_nnls_workgroup", C.c_int, [C.c_int, C.POINTER(C.c_int), C.POINTER(C.c_size_t), C.POINTER(C.c_int)]),
    ("t2fit_nnls_pack_bytes", C.c_int, [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_size_t)]),
    ("t2fit_nnls_pack_host", C.c_int, [C.c_int, C.c_int, C.c_int, _P, C.c_double, _P, _P, C.c_size_t]),
    ("t2fit_nnls_dev", C.c_int, [C.POINTER(T2FitNnlsParams), _P, C.c_int, C.c_int64, _P, _P, _P, _P, _P, _P, _P, _P, _P]),
    ("t2fit_nnls_chi2_params_default", C.c_int, [C.POINTER(T2FitNnlsChi2Params)]),
    ("t2fit_nnls_chi2_dev", C.c_int, [C.POINTER(T2FitNnlsParams), C.POINTER(T2FitNnlsChi2Params), _P, C.c_int, C.c_int64, _P, _P, _P, _P, _P, _P,
                                      _P, _P, _P, _P, _P, _P, _P]),
    ("t2fit_set_timing", C.c_int, [C.c_int]),
    ("t2fit_set_reserve_cus", C.c_int, [C.c_int]),
    ("t2fit_kernel_ms", C.c_double, [C.c_int]),
    ("t2fit_last_kernel_ms", C.c_double, []),
    ("t2fit_epilogue_ms", C.c_double, [C.c_int]),
    ("t2fit_last_error", C.c_char_p, []),
    ("t2fit_abi_version", C.c_int, []),
]


# entry points added to ABI 5 after its first release, by stage: another build of the same ABI (T2FIT_LIB) may lack them
BOOT_SYMBOLS = ("t2fit_boot_background_dev", "t2fit_boot_synth_dev", "t2fit_bootstrap_dev")
TV_SYMBOLS = ("t2fit_tv_params_default", "t2fit_tv_workspace_bytes", "t2fit_tv_denoise_dev")
RECON_SYMBOLS = ("t2fit_resample_dev", "t2fit_reconstruct_workspace_bytes", "t2fit_reconstruct_dev")
MORPH_SYMBOLS = ("t2fit_morph_workspace_bytes", "t2fit_binary_threshold_dev", "t2fit_binary_morph_dev", "t2fit_fill_holes_dev",
                 "t2fit_seed_labels_dev", "t2fit_relabel_dev")
ADDITIVE = BOOT_SYMBOLS + TV_SYMBOLS + RECON_SYMBOLS + MORPH_SYMBOLS
REGISTER_SYMBOLS = ("t2fit_register_workspace_bytes", "t2fit_register_sums_dev", "t2fit_shrink_dev", "t2fit_shrink_mask_dev")
ATLAS_SYMBOLS = ("t2fit_register_bin_dev", "t2fit_register_binned_workspace_bytes", "t2fit_register_binned_sums_dev",
                 "t2fit_register_sums_lut_dev")
N4_SYMBOLS = ("t2fit_n4_workspace_bytes", "t2fit_n4_log_dev", "t2fit_n4_minmax_dev", "t2fit_n4_histogram_dev", "t2fit_n4_weights_dev",
              "t2fit_n4_fit_dev", "t2fit_n4_field_dev", "t2fit_n4_apply_dev")
MI_SYMBOLS = ("t2fit_register_joint_hist_dev", "t2fit_register_mi_workspace_bytes", "t2fit_register_mi_gradient_dev")
SR_SYMBOLS = ("t2fit_sr_plan_host", "t2fit_sr_workspace_bytes", "t2fit_sr_forward_dev", "t2fit_sr_adjoint_dev")
SR_SLICE_SYMBOLS = ("t2fit_sr_slice_table_bytes", "t2fit_sr_slice_table_host", "t2fit_sr_slice_forward_dev",
                    "t2fit_sr_slice_adjoint_dev")
SVR_SYMBOLS = ("t2fit_svr_table_bytes", "t2fit_svr_table_host", "t2fit_svr_workspace_bytes", "t2fit_svr_sums_dev")
SR_ROBUST_SYMBOLS = ("t2fit_sr_robust_params_default", "t2fit_sr_robust_workspace_bytes", "t2fit_sr_robust_dev")
TVJ_SYMBOLS = ("t2fit_tv_joint_workspace_bytes", "t2fit_tv_joint_denoise_dev")
MPPCA_SYMBOLS = ("t2fit_mppca_params_default", "t2fit_mppca_workspace_bytes", "t2fit_mppca_dev")
SEG_SYMBOLS = ("t2fit_seg_workspace_bytes", "t2fit_seg_mask_dev", "t2fit_seg_priors_dev", "t2fit_seg_normalise_dev", "t2fit_seg_sums_dev",
               "t2fit_seg_estep_dev", "t2fit_seg_labels_dev")
FFD_SYMBOLS = ("t2fit_ffd_workspace_bytes", "t2fit_ffd_joint_hist_dev", "t2fit_ffd_gradient_dev", "t2fit_ffd_warp_dev",
               "t2fit_ffd_jacobian_dev")
DICT_SYMBOLS = ("t2fit_dict_pack_bytes", "t2fit_dict_pack_host", "t2fit_dict_match_dev")
UNRING_SYMBOLS = ("t2fit_unring_params_default", "t2fit_unring_tables_bytes", "t2fit_unring_tables_host", "t2fit_unring_workspace_bytes",
                  "t2fit_unring_split_dev", "t2fit_unring_rows_dev", "t2fit_unring_dev")
COMPONENT_SYMBOLS = ("t2fit_components_workspace_bytes", "t2fit_components_label_dev", "t2fit_components_stats_dev",
                     "t2fit_components_lut_dev")
EDT_SYMBOLS = ("t2fit_edt_workspace_bytes", "t2fit_edt_dev", "t2fit_edt_fill_dev")
NNLS_SYMBOLS = ("t2fit_nnls_params_default", "t2fit_nnls_workgroup", "t2fit_nnls_pack_bytes", "t2fit_nnls_pack_host", "t2fit_nnls_dev")
NNLS_CHI2_SYMBOLS = ("t2fit_nnls_chi2_params_default", "t2fit_nnls_chi2_dev")
LOOKED_UP = (ADDITIVE + REGISTER_SYMBOLS + ATLAS_SYMBOLS + N4_SYMBOLS + MI_SYMBOLS + SR_SYMBOLS + SR_SLICE_SYMBOLS + SVR_SYMBOLS
             + SR_ROBUST_SYMBOLS + TVJ_SYMBOLS + MPPCA_SYMBOLS + SEG_SYMBOLS + FFD_SYMBOLS + DICT_SYMBOLS + UNRING_SYMBOLS
             + COMPONENT_SYMBOLS + EDT_SYMBOLS + NNLS_SYMBOLS + NNLS_CHI2_SYMBOLS)


def bind(lib: C.CDLL) -> C.CDLL:
    """Attach prototypes; raises AttributeError if the library lacks a declared symbol (the LOOKED_UP ones are looked
    up: a library without them binds, and the stage that needs one raises when it is called)."""
    for name, res, args in SYMBOLS:
        if name in LOOKED_UP and not hasattr(lib, name):
            continue
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    return lib
