"""fetal_t2mapping_amd -- MI355X-native per-voxel T2 relaxation fit.

Drop-in for the voxel-wise fitting path of Medical-Image-Analysis-Laboratory/fetal_t2mapping
(run_t2mapping.py fit_voxel / process_t2maps + utils/t2map_utils.compute_residuals).  The fit runs
in hand-written HIP kernels (csrc/) behind the C ABI of include/t2fit.h; this package is the
Python host side that mirrors the reference's function surface.  There is no CPU execution path.
"""
from ._philox import philox4x32_10
from .t2map import (BootMaps, BootStats, RoiStats, T2Maps, bootstrap_volume, compute_residuals, denoise_tv, dense_labels,
                    estimate_background_sigma, fit_table, fit_volume, fit_voxel, fit_voxels, fit_voxels_trace, label_stats,
                    make_config, reconstruct_stacks, resample_volume, roi_erode, roi_frame, roi_stats, roi_table,
                    set_fit_params, stack_mask_flatten, synth_replica, union_mask_dev)
from .t2map import register  # the registrations: register.register_rigid, register.register_affine, register.registration_sums
from .t2map import atlas  # the atlas-label stage: atlas.atlas_labels, atlas.extract_brain
from .t2map import bias  # the N4 bias-field correction: bias.n4_correct, bias.apply_field
from .t2map import (binary_close, binary_dilate, binary_erode, binary_open, binary_threshold, build_mask, fill_holes,
                    mask_from_labels, phantom_labels, phantom_mask, relabel, seed_labels, synthseg_to_feta)
from .t2map import sr  # the super-resolution reconstruction: sr.reconstruct_sr, sr.sr_forward, sr.sr_adjoint, sr.sr_box
from ._gpu_sr import reconstruct_sr, sr_adjoint, sr_box, sr_forward  # the same four, by their own names
from ._gpu_sr import sr_adjoint_slices, sr_forward_slices, sr_slice_table  # the operators with a rigid pose per slice
from .t2map import mppca  # MP-PCA denoising and noise maps across the echoes: mppca.denoise_mppca, mppca.mppca_noise_map
from ._gpu_mppca import denoise_mppca, mppca_noise_map  # the same two, by their own names
from .t2map import seg  # atlas-prior EM tissue segmentation: seg.segment_em, seg.priors_from_labels (not in __all__, as t2map's own names are)
from .t2map import dictionary  # the dictionary-matching fit: dictionary.Dictionary, .monoexp, .biexp, .match, .fit_volume_dict (not in __all__)
from .t2map import components  # connected components: components.label, .stats, .select, .keep_largest, .remove_small, .reassign_small, .seeds (not in __all__)
from .t2map import distance  # the exact Euclidean distance transform: distance.nearest, .edt, .fill_nearest, .dilate_mm, .erode_mm, .surface, .surface_distances (not in __all__)
from .t2map import spectrum  # T2 spectra by regularised NNLS: spectrum.Basis, .spectrum_basis, .solve, .solve_chi2, .fit_volume_nnls (not in __all__)
from .t2map import unring  # Gibbs-ringing removal: unring.unring_volume, .unring_slices, .unring_split, .unring_rows, .unring_tables (not in __all__)

__all__ = ["BootMaps", "BootStats", "RoiStats", "T2Maps", "bootstrap_volume", "compute_residuals", "denoise_tv", "dense_labels",
           "estimate_background_sigma", "fit_table", "fit_volume", "fit_voxel", "fit_voxels", "fit_voxels_trace", "label_stats",
           "make_config", "philox4x32_10", "reconstruct_stacks", "resample_volume", "roi_erode", "roi_frame", "roi_stats", "roi_table", "set_fit_params",
           "stack_mask_flatten", "synth_replica", "union_mask_dev",
           "binary_close", "binary_dilate", "binary_erode", "binary_open", "binary_threshold", "build_mask", "fill_holes",
           "mask_from_labels", "phantom_labels", "phantom_mask", "relabel", "seed_labels", "synthseg_to_feta", "register",
           "atlas", "bias", "sr", "mppca"]
