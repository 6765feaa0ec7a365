"""Host-side mirror of the reference's fitting interface, backed by the HIP library.

Same names, argument meaning and error behaviour as the reference's hot path:

=============================  ================================================================
this module                    reference (paths relative to its root)
=============================  ================================================================
``set_fit_params(args)``       run_t2mapping.py:29-111
``fit_voxel(...)``             run_t2mapping.py:120-312 (one voxel; same 5-tuple)
``fit_voxels(...)``            the ``Pool.map`` over ``fit_voxel`` (:430-443), batched
``stack_mask_flatten(...)``    run_t2mapping.py:383-386,411-421
``fit_volume(...)``            run_t2mapping.py:411-461 (flatten, fit, scatter, residual map)
``compute_residuals(...)``     utils/t2map_utils.py:62-89
=============================  ================================================================

This module is the facade every caller goes through; the bindings live one module per stage, each beside the numpy
statement of what its kernels compute:

=====================  ==================  ===========================================================
stage                  binding             numpy definition
=====================  ==================  ===========================================================
fit, residual map      ``_gpu_fit``        (the reference itself; ``oracle/`` for the tests)
ROI statistics         ``_gpu_roi``        (numpy / scipy calls named in the docstrings)
bootstrap              ``_gpu_boot``       ``_philox``
TV denoising           ``_gpu_tv``         ``_tv``
MP-PCA denoising,      ``_gpu_mppca``      ``_mppca``; here as ``mppca``, and ``denoise_mppca`` / ``mppca_noise_map`` by name
noise maps
resampling, merge      ``_gpu_resample``   ``_resample``
masks, phantom labels  ``_gpu_morph``      ``_morph``
rigid registration     ``_gpu_register``   ``_register`` (and the optimizer, which is host code); here as ``register``
atlas labels           ``_gpu_atlas``      ``_atlas`` (affine registration by the correlation ratio: ``register``); here as ``atlas``
super-resolution       ``_gpu_sr``         ``_sr`` (operator, adjoint and the proximal-gradient loop; the prox is ``_tv``); here as ``sr``
slice-to-volume        ``_gpu_register``,  ``_svr`` (batched per-slice sums, transform model, lockstep descent and driver, which are host
registration           ``_gpu_sr``         code); here as ``register.register_slices``, ``register.slice_sums``, ``sr.reconstruct_svr``
tissue segmentation    ``_gpu_seg``        ``_seg`` (the steps, and the EM loop and class model, which are host code); here as ``seg``
dictionary fit         ``_gpu_dict``       ``_dict`` (and the dictionary builders, which both share); here as ``dictionary``
Gibbs-ringing removal  ``_gpu_unring``     ``_unring`` (and the tables, which both read); here as ``unring``
connected components   ``_gpu_components`` ``_components``; here as ``components``
distance transform     ``_gpu_edt``        ``_edt`` (and the surface measures' reductions, which are host code); here as ``distance``
T2 spectra (NNLS)      ``_gpu_nnls``       ``_nnls`` (and the basis and functional builders, which both share); here as ``spectrum``
N4 bias field          ``_gpu_bias``       ``_bias`` (and the sharpening table, the refinement and the loop, which are host code); here as ``bias``
=====================  ==================  ===========================================================

Python only marshals buffers (``_gpu``: conversions, ``out=`` checks, stream, workspace); all arithmetic happens in
libt2fit_hip.so through the C ABI of include/t2fit.h.  torch is used for device buffers and streams, nothing else.
"""
from ._gpu_boot import BootMaps, BootStats, bootstrap_volume, estimate_background_sigma, synth_replica  # noqa: F401
from ._gpu_fit import (T2Maps, compute_residuals, fit_table, fit_volume, fit_voxel, fit_voxels, fit_voxels_trace,  # noqa: F401
                       label_stats, make_config, set_fit_params, stack_mask_flatten, union_mask_dev)
from ._gpu_morph import (binary_close, binary_dilate, binary_erode, binary_open, binary_threshold, build_mask,  # noqa: F401
                         fill_holes, mask_from_labels, phantom_labels, phantom_mask, relabel, seed_labels, synthseg_to_feta)
from . import _gpu_atlas as atlas  # noqa: F401  (a namespace: atlas.atlas_labels, atlas.extract_brain)
from . import _gpu_bias as bias  # noqa: F401  (a namespace: bias.n4_correct, bias.apply_field, the step functions)
from . import _gpu_register as register  # noqa: F401  (a namespace: register.register_rigid, .register_affine, ..)
from ._gpu_resample import RECON_FORMS, reconstruct_stacks, resample_volume  # noqa: F401
from ._gpu_roi import ROI_MAX_LABELS, RoiStats, dense_labels, roi_erode, roi_frame, roi_stats, roi_table  # noqa: F401
from . import _gpu_sr as sr  # noqa: F401  (a namespace: sr.reconstruct_sr, sr.sr_forward, sr.sr_adjoint, sr.sr_box and, with a
#                               rigid pose per slice, sr.sr_forward_slices, sr.sr_adjoint_slices, sr.sr_slice_table; the
#                               outlier weighting of reconstruct_sr(robust=...) alone: sr.sr_robust_weights)
from ._gpu_tv import denoise_tv, tv_params  # noqa: F401
from . import _gpu_mppca as mppca  # noqa: F401  (a namespace: mppca.denoise_mppca, mppca.mppca_noise_map, mppca.mppca_params)
from . import _gpu_seg as seg  # noqa: F401  (a namespace: seg.segment_em, seg.priors_from_labels, seg.moment_sums, seg.e_step,
#                                seg.hard_labels, seg.seg_params)
from . import _gpu_dict as dictionary  # noqa: F401  (a namespace: dictionary.Dictionary, .monoexp, .biexp, .log_grid, .pack, .match,
#                                         .fit_volume_dict)
from . import _gpu_unring as unring  # noqa: F401  (a namespace: unring.unring_volume, .unring_slices, .unring_split, .unring_rows,
#                                       .unring_tables)
from . import _gpu_components as components  # noqa: F401  (a namespace: components.label, .stats, .lut, .select, .keep_largest,
#                                               .remove_small, .reassign_small, .seeds, .TILE)
from . import _gpu_edt as distance  # noqa: F401  (a namespace: distance.nearest, .edt, .fill_nearest, .dilate_mm, .erode_mm, .surface,
#                                      .surface_distances)
from . import _gpu_nnls as spectrum  # noqa: F401  (a namespace: spectrum.Basis, .spectrum_basis, .monoexp_basis, .window_functionals,
#                                        .ln_t2_functional, .log_grid, .pack, .solve, .fit_volume_nnls)


def __getattr__(name):
    """``t2map.denoise_mppca`` and ``t2map.mppca_noise_map``: the two entry points of the ``mppca`` namespace by their own
    names.  (Stages added after the split hang off namespaces; the set of names this module binds itself is the one the
    mirror test lists.)"""
    if name in ("denoise_mppca", "mppca_noise_map"):
        return getattr(mppca, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
