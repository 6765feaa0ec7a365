/*
 * t2fit.h -- C ABI of the MI355X per-voxel T2 relaxation fitter (libt2fit_hip.so).
 *
 * This is the drop-in boundary for ONE hot path of Medical-Image-Analysis-Laboratory/
 * fetal_t2mapping: the voxel-wise fit that run_t2mapping.py drives.  The reference has no FFI of
 * its own (it is pure Python); each entry point below names the Python call site it replaces
 * (paths relative to the reference root).  Plain pointers and sizes only: no Python, torch or
 * C++ types cross this boundary.  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *   - all functions return 0 on success, a negative T2FIT_E_* code otherwise; the message of the
 *     last failure on the calling thread is available from t2fit_last_error().
 *   - "dev" pointers are HIP device pointers (e.g. torch.Tensor.data_ptr() on ROCm); "host"
 *     pointers are ordinary memory.  `stream` is a hipStream_t passed as void* (NULL = default).
 *   - echo samples are float32; echo times, tables and tolerances are float64 in MILLISECONDS,
 *     as everywhere in the reference (run_t2mapping.py:369).
 *   - n_vox is the dense voxel count N = Z*Y*X (C order, run_t2mapping.py:411); masked-out voxels
 *     are written as zeros in every map (run_t2mapping.py:415-418).
 */
#ifndef T2FIT_H
#define T2FIT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define T2FIT_ABI_VERSION 5
#define T2FIT_MAX_TE 32

/* error codes */
#define T2FIT_OK 0
#define T2FIT_E_INVALID (-1) /* bad argument (null pointer, size, unknown enum)            */
#define T2FIT_E_HIP (-2)     /* a HIP runtime call failed (no device, OOM, launch failure) */
#define T2FIT_E_BOUNDS (-3)  /* table bounds have lb > ub (scipy raises ValueError there)  */

/* objective, run_t2mapping.py:129-177 */
#define T2FIT_MODEL_GAUSSIAN 0        /* mean (y - k e^{-t/T2})^2                    :141-147 */
#define T2FIT_MODEL_GAUSSIAN_RICIAN 1 /* mean (y - sqrt(k^2 e^{-2t/T2} + s^2))^2     :149-155 */
#define T2FIT_MODEL_RICIAN 2          /* Rician negative log-likelihood with i0e     :157-177 */

/* solver */
#define T2FIT_SOLVER_LBFGSB 0 /* the reference's solver and stop rules: per-lane L-BFGS-B (m=10) with
                                 scipy's bound-aware forward-difference gradient, float64
                                 (run_t2mapping.py:260-286 -> scipy.optimize.minimize)             */
#define T2FIT_SOLVER_LM 1     /* log-linear seed + bounded Levenberg-Marquardt run to convergence of
                                 the same objective and bounds (least-squares models only)          */

#define T2FIT_SOLVER_LOGLIN 2 /* closed-form weighted log-linear regression ln y = ln k - t/T2 (weights
                                 y^2), clipped into the same bounds; 2-parameter model only; one pass,
                                 HBM-bound.  Extension named by BASELINE.json config 2: the reference
                                 has no log-linear routine (parity with it is unpinned)               */

/* arithmetic of the LM solver (the L-BFGS-B solver is always float64) */
#define T2FIT_PREC_F64 0
#define T2FIT_PREC_F32 1

/* memory layout of the echo stack */
#define T2FIT_LAYOUT_TE_MAJOR 0    /* (nTE, N): nTE contiguous volumes, what the reader produces
                                      before np.stack (run_t2mapping.py:377)                 */
#define T2FIT_LAYOUT_VOXEL_MAJOR 1 /* (N, nTE): the reference's reshaped_t2w (:411)          */

/* per-voxel status map values */
#define T2FIT_ST_MASKED 0     /* outside the mask, not fitted                                  */
#define T2FIT_ST_CONVERGED 1  /* solver's convergence test met (scipy result.success == True)  */
#define T2FIT_ST_NOT_CONV 2   /* iteration/evaluation cap or abnormal line-search termination  */
#define T2FIT_ST_NONFINITE 3  /* non-finite sample or objective at the start: x = clipped x0,
                                 nit = 0 (scipy: ABNORMAL, success False; run_t2mapping.py:298) */
#define T2FIT_ST_INFEASIBLE 4 /* data-dependent bounds with lb > ub (no-prior and S(TE0) > 10000):
                                 the reference raises ValueError and aborts the volume; maps get NaN */

/* Fit configuration: the reference's fit_params dict (run_t2mapping.py:29-111) plus the per-call
 * flags of fit_voxel (:120) flattened to a POD.  Fill with t2fit_config_default() first. */
typedef struct t2fit_config {
  int32_t abi_version;        /* T2FIT_ABI_VERSION */
  int32_t model;              /* T2FIT_MODEL_*                                     */
  int32_t solver;             /* T2FIT_SOLVER_*                                    */
  int32_t precision;          /* T2FIT_PREC_* (LM only)                            */
  int32_t n_te;               /* 2..T2FIT_MAX_TE                                   */
  int32_t no_prior;           /* 1: k >= S(TE0), k <= 10000, T2 in [10,2000]  (:243-245)      */
  int32_t norm;               /* 1: divide each voxel's samples by their maximum (:237-238)    */
  int32_t maxls;              /* L-BFGS-B line-search step cap ("maxls", 50 in every table)    */
  int32_t maxiter;            /* iteration cap: scipy default 15000 (L-BFGS-B); LM default 60  */
  int32_t maxfun;             /* objective-evaluation cap (scipy default 15000)                */
  int32_t numpy_legacy;       /* 0 (default): float promotion of numpy >= 2 (NEP 50), what the image's numpy does.
                                 1: value-based casting of numpy < 2 -- the reference freezes numpy 1.26.0
                                 (requirements_frozen.txt:103).  Two places on the path differ: the rician
                                 objective's  np.log(signal) - np.log(sigma**2)  (run_t2mapping.py:169) is then a
                                 FLOAT32 subtraction, and the residual map's prediction  k_map * np.exp(-te / t2_map)
                                 (utils/t2map_utils.py:74-80) is float32 throughout.  (ABI 4; was reserved0.)   */
  int32_t reserved1;
  double te_ms[T2FIT_MAX_TE]; /* echo times [ms], ascending                                     */
  double x0[3];               /* initial_guess (k, T2, sigma); clipped into the bounds as scipy does */
  double lb[3];               /* param_bounds lower (k, T2, sigma)                              */
  double ub[3];               /* param_bounds upper                                             */
  double ftol;                /* L-BFGS-B relative-reduction stop (1e-6 / 1e-2 in the tables)  */
  double gtol;                /* L-BFGS-B projected-gradient stop (scipy default 1e-5 / 1e-2)  */
  double fd_step;             /* absolute forward-difference step, scipy "eps" = 1e-8          */
  double lm_xtol;             /* LM relative step tolerance (0 = default for the precision)    */
  double noprior_k_ub;        /* 10000 (:244) */
  double noprior_t2_lb;       /* 10    (:245) */
  double noprior_t2_ub;       /* 2000  (:245) */
} t2fit_config;

/* Output maps.  t2/k/sigma/res are the reference's four maps (utils/t2map_utils.py:18-29); the
 * others are optional (NULL = not wanted) and replace the per-voxel tuples fit_voxel returns
 * (run_t2mapping.py:312).  All arrays have n_vox elements. */
typedef struct t2fit_maps {
  float *t2;       /* result.x[1]  (run_t2mapping.py:456-458)                                   */
  float *k;        /* result.x[0]                                                               */
  float *sigma;    /* result.x[2]; zeros for the 2-parameter model                              */
  float *res;      /* mean signed residual over TE (utils/t2map_utils.py:84)                    */
  float *r2;       /* optional: 1 - SS_res/SS_tot about the mean (no reference map; extension)  */
  float *fun;      /* optional: final objective value (result.fun, :293)                        */
  int32_t *nit;    /* optional: iterations (result.nit, :292)                                   */
  uint8_t *status; /* optional: T2FIT_ST_*                                                      */
  float *t2_se;    /* optional: standard error of T2 [ms] from the Gauss-Newton covariance
                      s^2 (J^T J)^-1, s^2 = SS_res / (nTE - n_par), J = d model / d (k, T2, sigma) at the
                      float32 map values; NaN when nTE <= n_par or J^T J is singular.  A 95 % confidence
                      interval is T2 +- 1.96 t2_se.  Extension: the reference has no CI map.            */
} t2fit_maps;

/* Fill *cfg with the reference table for (model, low_field): x0, bounds, ftol/gtol/maxls from
 * run_t2mapping.py:38-106, scipy defaults for the rest, solver = L-BFGS-B.  Replaces
 * set_fit_params() (run_t2mapping.py:29-111). */
int t2fit_config_default(t2fit_config *cfg, int model, int low_field);

/* Number of HIP devices visible (0 when there is none; never fails). */
int t2fit_device_count(void);

/* Volume seam, device buffers: replaces run_t2mapping.py:427-461 (Pool.map over fit_voxel, the
 * scatter into maps and compute_residuals) for one (sub,ses).
 *   echoes_dev : float32, layout per `layout`
 *   mask_dev   : uint8 [n_vox] (non-zero = fit), or NULL to fit every voxel
 *   maps       : device pointers
 *   n_vox      : below 2^32 per call (split larger stacks into slabs; voxels are independent)
 * Asynchronous on `stream`; the caller synchronises.  Two launches: the persistent fit kernel
 * (t2, k, sigma and the optional per-voxel extras) and a streaming epilogue (res, r2, t2_se). */
int t2fit_volume_dev(const t2fit_config *cfg, const float *echoes_dev, int layout,
                     const uint8_t *mask_dev, int64_t n_vox, const t2fit_maps *maps, void *stream);

/* Context of the host seam: the state a sequence of numpy-in / numpy-out fits shares (run_t2mapping.py:358 fits one
 * (sub, ses) after the other): three HIP streams, recycled events, a grow-only device arena, two page-locked
 * staging slots per direction and a few copy threads (T2FIT_COPY_THREADS, default 8).  One call at a time per
 * context; contexts of different devices (or several per device) are independent. */
typedef struct t2fit_context t2fit_context;
int t2fit_create(int device, t2fit_context **out);
int t2fit_destroy(t2fit_context *ctx); /* waits for outstanding work; NULL is a no-op */

/* Volume seam, host buffers (numpy arrays): replaces run_t2mapping.py:411-461 for one (sub,ses).  The volume goes
 * through in slabs of about 2 M voxels: while one slab is fitted the worker threads copy the next one's samples from
 * the caller's (pageable) arrays into page-locked staging and the previous one's maps out of it, so the device only
 * DMAs from and to page-locked memory.  The maps do not depend on the split (voxels are independent).  Synchronous:
 * the maps are complete on return. */
int t2fit_context_volume_host(t2fit_context *ctx, const t2fit_config *cfg, const float *echoes, int layout,
                              const uint8_t *mask, int64_t n_vox, const t2fit_maps *maps);

/* The same without a context of the caller's: uses a per-device context that the library creates on first use
 * and keeps for the life of the process.  `device` = HIP device ordinal. */
int t2fit_volume_host(const t2fit_config *cfg, const float *echoes, int layout, const uint8_t *mask,
                      int64_t n_vox, const t2fit_maps *maps, int device);

/* Voxel seam (run_t2mapping.py:120 fit_voxel, batched): fit rows idx[0..n_idx) of the
 * (N, nTE) or (nTE, N) stack and return the per-voxel tuple fields densely packed:
 *   x[n_idx*3] float64 (k, T2, sigma; sigma = 0 for the 2-parameter model), fun[n_idx] float64,
 *   nit[n_idx], status[n_idx].  Host pointers. */
int t2fit_voxels_host(const t2fit_config *cfg, const float *echoes, int layout, int64_t n_vox,
                      const int64_t *idx, int64_t n_idx, double *x, double *fun, int32_t *nit,
                      uint8_t *status, int device);

/* The same with per-iteration traces -- what the reference's callbacks collect into
 * iteration_info (run_t2mapping.py:180-234) and its convergence plots consume:
 *   trace[n_idx * trace_cap * 4] float64: (k, T2, sigma, objective) after each iteration,
 *   trace_len[n_idx]: iterations recorded (<= trace_cap; later ones are dropped). */
int t2fit_voxels_trace_host(const t2fit_config *cfg, const float *echoes, int layout, int64_t n_vox,
                            const int64_t *idx, int64_t n_idx, double *x, double *fun, int32_t *nit,
                            uint8_t *status, int trace_cap, double *trace, int32_t *trace_len,
                            int device);

/* Union mask + flat indices: replaces run_t2mapping.py:383-384,412,421.
 *   masks_dev : n_masks volumes of uint8 [n_vox] each, contiguous (n_masks, n_vox)
 *   mask_out  : uint8 [n_vox], 1 where any input mask is non-zero
 *   idx_out   : int64 [n_vox] capacity; ascending flat indices of the union (np.where order)
 *   count_out : device int64, number of indices written
 * Asynchronous on `stream`. */
int t2fit_union_mask_dev(const uint8_t *masks_dev, int n_masks, int64_t n_vox, uint8_t *mask_out,
                         int64_t *idx_out, int64_t *count_out, void *stream);

/* Residual map alone: replaces compute_residuals (utils/t2map_utils.py:62-89) for maps that are
 * already on the device (all float32 [n_vox]). */
int t2fit_residuals_dev(const t2fit_config *cfg, const float *echoes_dev, int layout,
                        const uint8_t *mask_dev, int64_t n_vox, const float *t2, const float *k,
                        const float *sigma, float *res, void *stream);

/* Phantom ROI statistics: replaces the per-vial nanmean / nanstd loop of save_phantom_csv
 * (utils/t2map_utils.py:43-53) for a map that is on the device.
 *   map_dev   : float32 [n_vox]
 *   label_dev : int32 [n_vox]; voxels labelled 1..n_labels are tallied (n_labels <= 32), others ignored
 *   mean_out, std_out : device float64 [n_labels]: mean and population standard deviation (ddof = 0) over
 *               the non-NaN values of each label, NaN for a label without any (numpy's result)
 *   count_out : device int64 [n_labels] or NULL: number of non-NaN values per label
 * Asynchronous on `stream`; the result does not depend on the launch (fixed summation order). */
int t2fit_label_stats_dev(const float *map_dev, const int32_t *label_dev, int64_t n_vox, int n_labels,
                          double *mean_out, double *std_out, int64_t *count_out, void *stream);

/* In-vivo atlas ROIs, step 1: the eroded region of every label at once.  Replaces, for all labels L in 1..n_labels,
 *   binary_erosion((tissue == tissue_value) & (label == L), structure=generate_binary_structure(3, connectivity),
 *                  iterations=iterations)
 * of utils/ada_utils.py:165-169, :192-196 (get_t2_per_roi: Harvard-Oxford labels in FeTA grey matter, JHU labels in FeTA
 * white matter) and :925-933 (compute_t2_per_tissue_feta).  The masks of one atlas are disjoint, so all of them are eroded
 * by one stencil pass per iteration over the class volume  cls = (tissue == tissue_value) ? label : 0:  a voxel keeps its
 * class iff every neighbour of the element lies inside the volume and has the same class (scipy's border_value = 0: voxels
 * on the faces of the volume are always eroded).
 *   label_dev    : int32 [nz, ny, nx] (C order, x innermost); values outside 1..n_labels are background
 *   tissue_dev   : int32, same shape, or NULL (every voxel qualifies)
 *   n_labels     : 1..256
 *   connectivity : 1, 2, 3 = 6, 18, 26 neighbours (|dz| + |dy| + |dx| <= connectivity); the reference uses 3
 *   iterations   : 0..8; 0 = the class volume alone, no erosion
 *   roi_out      : int32 [nz * ny * nx]: the surviving class, or 0; must not be one of the inputs
 * nz * ny * nx below 2^32.  Asynchronous on `stream`; the result is a function of the inputs alone. */
int t2fit_roi_erode_dev(const int32_t *label_dev, const int32_t *tissue_dev, int32_t tissue_value, int nz, int ny, int nx,
                        int n_labels, int connectivity, int iterations, int32_t *roi_out, void *stream);

/* In-vivo atlas ROIs, step 2: np.mean / np.std / np.median / len of the map values of every region
 * (utils/ada_utils.py:171-189, :198-216, :935-960) for a map that is on the device.
 *   map_dev    : float32 [n_vox]
 *   roi_dev    : int32 [n_vox], e.g. roi_out of t2fit_roi_erode_dev; voxels with values 1..n_labels (<= 256) are tallied
 *   mean_out, std_out : device float64 [n_labels]: mean and population standard deviation (ddof = 0), numpy's two rounds
 *   median_out : device float64 [n_labels] or NULL: the exact median (the mean of the two middle values for an even count)
 *   count_out  : device int64 [n_labels]: voxels of the region (the reference's `nvoxel`)
 *   valid_out  : device int64 [n_labels] or NULL: those whose map value is not NaN
 * The statistics are over the non-NaN values, as in t2fit_label_stats_dev (np.mean of a region holding a NaN -- a
 * T2FIT_ST_INFEASIBLE voxel -- is NaN in the reference; count_out != valid_out tells the caller so); a region without
 * any gives NaN.  n_vox in 1..2^32-1.  Asynchronous on `stream`; two calls on the same inputs return the same bits, on
 * any launch geometry (integer counting sort in voxel order, fixed summation tree, exact selection). */
int t2fit_roi_stats_dev(const float *map_dev, const int32_t *roi_dev, int64_t n_vox, int n_labels, double *mean_out,
                        double *std_out, double *median_out, int64_t *count_out, int64_t *valid_out, void *stream);

/* ---- Parametric bootstrap: per-voxel bias / standard deviation / percentile interval of the fit as it is run --------
 * No reference counterpart (the reference has no uncertainty map).  The acquisition is simulated from the fitted (k, T2)
 * with noise of a given level, refitted by t2fit_volume_dev with the same cfg (solver, bounds, prior, stop rules) and
 * mask, R times; the distribution of the R refits of every voxel is reduced on the device.  Additive to ABI 5: new
 * symbols and one new struct, t2fit_config and t2fit_maps are as they were (look the symbols up to detect them).
 * cfg.norm = 1 is refused by all of them: the maps of a normalised fit are in per-voxel units of the largest sample,
 * and the noise level would have to be too.
 *
 * The replica stream (the definition; fetal_t2mapping_amd/_philox.py restates it in numpy):
 *   (w0, w1, w2, w3) = Philox4x32-10(counter = (v low, v high, j, r), key = (seed low, seed high))
 *       v = voxel_offset + flat index of the voxel, j = echo, r = replica; w2 and w3 are not used
 *   u1 = ((w0 >> 9) + 0.5) 2^-23,  u2 = ((w1 >> 9) + 0.5) 2^-23      (exact in float32, never 0 or 1)
 *   n1 = sqrt(-2 ln u1) cos(2 pi u2),  n2 = sqrt(-2 ln u1) sin(2 pi u2)          (|n| <= 5.77)
 *   S = k[v] exp(-TE[j] / T2[v]),  s = noise level of the voxel
 *   sample = sqrt((S + s n1)^2 + (s n2)^2)  (T2FIT_BOOT_NOISE_RICIAN)   or   S + s n1  (T2FIT_BOOT_NOISE_GAUSSIAN)
 * evaluated in float32.  A sample depends on (seed, v, j, r) alone: not on the launch, the mask, a slab partition or the
 * order of the replicas. */
#define T2FIT_BOOT_NOISE_RICIAN 0
#define T2FIT_BOOT_NOISE_GAUSSIAN 1

#define T2FIT_BOOT_PARAM_T2 1 /* which_params: a set of these; index into t2fit_boot_maps = 0, 1, 2 */
#define T2FIT_BOOT_PARAM_K 2
#define T2FIT_BOOT_PARAM_SIGMA 4

/* Output maps of t2fit_bootstrap_dev: device float32 [n_vox] each, index 0 = T2, 1 = k, 2 = sigma; NULL = not wanted.
 * Zeros outside the mask.  With n_ok counted replicas of the voxel: mean and bias = mean - fitted value (NaN when
 * n_ok = 0), std with ddof = 1 (NaN when n_ok < 2), ci_lo / ci_hi = numpy's default ("linear") percentiles at
 * 100 alpha / 2 and 100 (1 - alpha / 2) of the counted replicas (NaN when n_ok = 0).  The call is in interval mode when
 * a ci_lo or ci_hi pointer of a requested parameter is set.
 * A fitted value that is not finite (T2 = +inf of a flat signal, or NaN, in a map handed in) does not spoil the
 * statistics of the replicas: mean, std and the percentiles are those of the counted refits, which are finite; only
 * bias = mean - fitted value follows IEEE arithmetic (-inf for +inf, NaN for NaN).  Internally the sums are taken about
 * the fitted value when it is finite and about 0 otherwise. */
typedef struct t2fit_boot_maps {
  float *mean[3];
  float *bias[3];
  float *std[3];
  float *ci_lo[3];
  float *ci_hi[3];
  int32_t *n_ok; /* int32 [n_vox]: replicas that count: status T2FIT_ST_CONVERGED and every requested value finite */
} t2fit_boot_maps;

/* Noise level from the background: sigma = sqrt(sum S^2 / (2 M)) over the M samples (all echoes) of the voxels whose
 * mask is 0 -- the second moment of the Rayleigh distribution a magnitude image has where there is no signal (what the
 * reference's unused estimate_in_vitro_noise, utils/t2map_utils.py:92-112, reaches for).  float64, fixed summation tree:
 * the same bits from call to call.  mask_dev is required; M = 0 is T2FIT_E_INVALID.  *sigma_out, *count_out are HOST
 * pointers; the call waits for `stream`. */
int t2fit_boot_background_dev(const float *echoes_dev, int layout, const uint8_t *mask_dev, int n_te, int64_t n_vox,
                              double *sigma_out, int64_t *count_out, void *stream);

/* One replica of the acquisition (the stream defined above), as a dense te-major (n_te, n_vox) float32 block that
 * t2fit_volume_dev fits as it stands; unmasked voxels are written as 0.
 *   t2_dev, k_dev  : the fitted maps, float32 [n_vox]
 *   noise_scalar   : the noise level s, used when noise_map_dev is NULL; noise_map_dev: float32 [n_vox], s per voxel
 *   mask_dev       : uint8 [n_vox] or NULL (every voxel)
 *   voxel_offset   : flat index of this block's voxel 0 in the volume the stream is defined on (0 for a whole volume;
 *                    z0 * ny * nx for a slab, which then equals the same rows of the whole volume bit for bit)
 * Uses cfg for n_te and te_ms only (and refuses cfg.norm).  Asynchronous on `stream`. */
int t2fit_boot_synth_dev(const t2fit_config *cfg, const float *t2_dev, const float *k_dev, double noise_scalar,
                         const float *noise_map_dev, const uint8_t *mask_dev, int64_t n_vox, int64_t voxel_offset,
                         uint64_t seed, int replica, int noise_kind, float *echoes_out_dev, void *stream);

/* The whole loop: for r in 0..n_replicas-1  synthesise replica r -> t2fit_volume_dev(cfg) -> accumulate, then finalise
 * into `out`.  Two replica blocks and two streams: replica r + 1 is synthesised while replica r is fitted.
 *   ctx          : its streams are used (one call at a time per context), or NULL: two streams are made for the call
 *   sigma_dev    : the fitted sigma map, needed (non-NULL) only with T2FIT_BOOT_PARAM_SIGMA, which the 2-parameter
 *                  gaussian model refuses
 *   mask_dev     : required (a mask of ones takes every voxel)
 *   n_replicas   : >= 1; in interval mode 2..512 (the values of 64 voxels are staged on chip for the rank select)
 *   alpha        : in (0, 1) in interval mode, e.g. 0.05 for a 95 % interval
 *   flags        : reserved, must be 0
 * Arguments are checked, and the workspace is sized and compared with the free device memory, before any device work;
 * it is allocated once per call and freed on every way out:
 *   n_vox (8 n_te + 26) + n_masked (4 + n_par (24 + 4 n_replicas [interval mode]))  bytes
 * (the check bounds n_masked by n_vox: the mask has not been read yet; the environment variable T2FIT_BOOT_MEM_LIMIT, in
 * bytes, caps what a call may take whatever is free, and is compared before the HIP runtime is touched).  Synchronous: work queued on `stream` before the
 * call is waited for, and the maps are complete on return.  Results are a function of the arguments alone. */
int t2fit_bootstrap_dev(t2fit_context *ctx, const t2fit_config *cfg, const float *t2_dev, const float *k_dev,
                        const float *sigma_dev, double noise_scalar, const float *noise_map_dev, int noise_kind,
                        const uint8_t *mask_dev, int64_t n_vox, int n_replicas, uint64_t seed, double alpha,
                        int which_params, const t2fit_boot_maps *out, int flags, void *stream);

/* ---- Total-variation denoising of the echo stack, ahead of the fit ---------------------------------------------------
 * The reference's reconstruction stage ends with run_denoising (utils/qmri_utils.py:393-405): every slice of every echo
 * volume goes through skimage.restoration.denoise_tv_chambolle (scikit-image 0.22, its defaults) before run_t2mapping.py
 * reads the file.  This is that function on the device for a float32 stack (n_vol, nz, ny, nx), x innermost.  Additive
 * to ABI 5: three new symbols and one new struct (look the symbols up to detect them).
 *
 * One problem is one (ny, nx) slice (dims = 2: n_vol * nz problems) or one (nz, ny, nx) volume (dims = 3: n_vol
 * problems); problems are independent.  For a problem f with n = dims axes (in memory order, x last) and N elements, in
 * the working precision T, tau = 1 / (2 n):
 *   p_a = 0 for every axis a
 *   for i = 0 .. max_iter - 1:
 *     d[x]   = 0 if i == 0, else ((-(p_0 + .. + p_{n-1})[x]) + p_0[x - e_0]) + p_1[x - e_1] ..   (axis order; a term is
 *              dropped where x - e_a is outside)
 *     out    = f + d
 *     g_a[x] = out[x + e_a] - out[x]   (0 where x + e_a is outside)
 *     nrm    = sqrt((g_0^2 + g_1^2) (+ g_2^2))
 *     E      = (sum d^2 + weight * sum nrm) / N
 *     p_a    = (p_a - T(tau) * g_a) / (1 + T(tau / weight) * nrm)
 *     i == 0: E_init = E_prev = E;  else if |E_prev - E| < eps * E_init: stop;  else E_prev = E
 *   result = out of the last iteration executed; n_iter = i at a stop, max_iter - 1 when the loop runs out
 * Every elementwise operation is one correctly rounded operation in T, in the order written (no fused multiply-add).
 * The squares d^2 and the norms are formed in T and summed in float64 in a fixed tree (E is float64: skimage sums in
 * the image's precision, so on a float32 image its stop can fall one iteration away when |E_prev - E| lies within
 * float32 rounding of the threshold); the stop iteration and every output byte are the same from call to call.
 * precision = T2FIT_PREC_F32 iterates in float32 (skimage on a float32 image); T2FIT_PREC_F64 widens the input,
 * iterates in float64 and rounds `out` to float32 once at the end (the reference: float64 reconstruction, the file is
 * read back as float32).  eps = 0 never stops early.  fetal_t2mapping_amd/_tv.py restates the loop in numpy. */
typedef struct t2fit_tv_params {
  double weight;     /* > 0, in intensity units of the stack (skimage does not rescale a float image) */
  double eps;        /* >= 0 */
  int32_t max_iter;  /* >= 1 */
  int32_t dims;      /* 2 or 3 */
  int32_t precision; /* T2FIT_PREC_F32 or T2FIT_PREC_F64 */
  int32_t flags;     /* reserved, must be 0 */
} t2fit_tv_params;

/* skimage's defaults, hence the reference's: weight 0.1, eps 2e-4, max_iter 200; dims 2, T2FIT_PREC_F32, flags 0 */
int t2fit_tv_params_default(t2fit_tv_params *p);

/* Bytes of the workspace a call needs; plain arithmetic, no device.  With e = 4 (F32) or 8 (F64) bytes, up(v) = v
 * rounded up to a multiple of 256, problems as above and tiles of 32 x 64 (dims = 2: ceil(ny / 32) ceil(nx / 64) per
 * problem) or 4 x 8 x 64 (dims = 3: ceil(nz / 4) ceil(ny / 8) ceil(nx / 64) per problem):
 *   2 up(dims * n_vol * nz * ny * nx * e)  [the two halves of the p pair]  +  up(16 * tiles)  [partial energies]
 *   +  up(32 * problems)  [E_init, E_prev, E, done flag, n_iter of every problem]
 * Refuses what t2fit_tv_denoise_dev refuses in p and the sizes: a size < 1, more than 2^40 elements (the voxel index is
 * 64-bit, the byte counts stay far inside size_t), more than 2^31-1 tiles (the launch index is 32-bit). */
int t2fit_tv_workspace_bytes(const t2fit_tv_params *p, int n_vol, int nz, int ny, int nx, size_t *bytes);

/* Denoise in_dev into out_dev (both device float32 [n_vol * nz * ny * nx]; out_dev == in_dev is allowed, a partial
 * overlap is not).  workspace_dev: at least t2fit_tv_workspace_bytes bytes, aligned to 256; its contents on entry do not
 * matter and it may be reused or freed once the stream has passed the call.  n_iter_dev (int32) / energy_dev (float64,
 * E of the last iteration executed): one per problem in memory order, or NULL.  A 1-wide axis is legal (its difference
 * is 0).  NaN / Inf in a problem stay in that problem (it runs max_iter iterations: no comparison with NaN stops it).
 * Asynchronous on `stream`: 2 max_iter + 1 launches are queued, the stop rule runs on the device and the workgroups of a
 * finished problem return at once; no allocation, free, copy or synchronisation inside.  Every argument is checked
 * before HIP is touched (T2FIT_E_INVALID and a message): NULL p / in_dev / out_dev / workspace_dev, weight <= 0 or not
 * finite, eps < 0 or not finite, max_iter < 1, dims not 2 / 3, unknown precision, flags != 0, a size < 1 or too large
 * (above), a workspace that is too small or not aligned to 256 bytes, a stack pointer not aligned to 4 bytes.
 * 128-bit accesses are used when nx % 4 == 0 and the stack pointers are 16-byte aligned; anything else takes
 * element-wise accesses and gives the same bits. */
int t2fit_tv_denoise_dev(const t2fit_tv_params *p, const float *in_dev, float *out_dev, int n_vol, int nz, int ny, int nx,
                         void *workspace_dev, size_t workspace_bytes, int32_t *n_iter_dev, double *energy_dev, void *stream);

/* ---- Vector-valued (joint) TV across the channels of the stack ---------------------------------------------------------
 * The scalar call above treats every echo as an image of its own, so edges land at different voxels at different echo
 * times.  The joint form couples the C = n_chan channels (echo times) of the float32 stack (n_chan, nz, ny, nx), the
 * te-major stack t2fit_tv_denoise_dev and t2fit_volume_dev take, through one gradient norm per voxel,
 * sqrt(sum_c |grad u_c|^2): all channels share one edge set.  Additive to ABI 5: two new symbols, the struct is
 * t2fit_tv_params with flags == 0.
 *
 * dims = 2: a problem is slice z of all channels (nz problems; the channel stride is nz * ny * nx); dims = 3: the whole
 * stack is one problem.  With n = dims spatial axes, N = C * (spatial voxels of a problem), working precision T and
 * tau = 1 / (2 n) (unchanged: the bound ||div||^2 <= 4 n holds channel by channel):
 *   p_{c,a} = 0
 *   for i = 0 .. max_iter - 1:
 *     d_c     = 0 if i == 0, else the scalar definition's divergence of (p_{c,0..n-1}): same order, same dropped terms
 *     out_c   = f_c + d_c
 *     g_{c,a}[x] = out_c[x + e_a] - out_c[x]   (0 where x + e_a is outside)
 *     sq_c    = (g_{c,0}^2 + g_{c,1}^2) (+ g_{c,2}^2)
 *     S       = sq_0;  S = S + sq_c for c = 1 .. C - 1, ascending
 *     nrm     = sqrt(S)                        (one per voxel, shared by all channels)
 *     E       = (sum_c sum_x d_c^2 + weight * sum_x nrm) / N
 *     p_{c,a} = (p_{c,a} - T(tau) * g_{c,a}) / (1 + T(tau / weight) * nrm)
 *     the stop rule on E and n_iter exactly as in the scalar definition
 *   result = out_c of the last iteration executed
 * Arithmetic as in the scalar definition: one correctly rounded operation in T per elementwise step, in the order
 * written, no fused multiply-add; d^2 and nrm formed in T and summed in float64 in a fixed tree (channels ascending
 * inside a tile).  With C = 1 every byte, n_iter and E are those of t2fit_tv_denoise_dev.  NaN / Inf in any channel of a
 * problem reaches every channel of that problem through nrm and stays inside that problem.
 * The weight is in intensity units and is NOT rescaled by C: the joint norm of pure noise is about sqrt(C) times a
 * channel's, so a weight that suits the scalar call is about sqrt(C) too small here.
 * fetal_t2mapping_amd/_tv.py (tv_joint_problem) restates the loop in numpy. */
#define T2FIT_TV_JOINT_MAX_CHAN 64 /* n_chan above this is refused (the kernels loop the channels: any count up to it runs) */

/* Bytes of the workspace of a joint call; plain arithmetic, no device.  With e, up() and the tiles of
 * t2fit_tv_workspace_bytes, problems = nz (dims = 2) or 1 (dims = 3) and tiles counted per problem over its spatial
 * extent (one tile serves all channels):
 *   2 up(dims * n_chan * nz * ny * nx * e)  [the p pair of all channels]  +  up(16 * tiles * problems)  [partial energies]
 *   +  up(32 * problems)  [state]
 * Refuses what t2fit_tv_joint_denoise_dev refuses in p and the sizes. */
int t2fit_tv_joint_workspace_bytes(const t2fit_tv_params *p, int n_chan, int nz, int ny, int nx, size_t *bytes);

/* The contract of t2fit_tv_denoise_dev: in place allowed, workspace aligned to 256 and of any content, n_iter_dev /
 * energy_dev one per problem or NULL, asynchronous on `stream` with 2 max_iter + 1 launches queued, the stop rule on the
 * device, no allocation, copy or synchronisation inside, every argument checked before HIP is touched with the same
 * refusals, and n_chan < 1 or > T2FIT_TV_JOINT_MAX_CHAN.  p->flags must be 0.  Per iteration a workgroup reads f and p
 * of every channel of its tile twice (once for S, once for the update; the last channel once) and writes p once. */
int t2fit_tv_joint_denoise_dev(const t2fit_tv_params *p, const float *in_dev, float *out_dev, int n_chan, int nz, int ny, int nx,
                               void *workspace_dev, size_t workspace_bytes, int32_t *n_iter_dev, double *energy_dev,
                               void *stream);

/* ---- Marchenko-Pastur PCA denoising and noise maps across the echoes (additive to ABI 5) ---------------------------
 * Veraart et al., NeuroImage 2016, as MRtrix's dwidenoise implements it: a denoiser with no weight to tune and a noise
 * map measured in tissue.  Over a window of N = (2 radius + 1)^dims voxels (x, y for dims = 2; x, y, z for dims = 3) the
 * n_te echoes form an n_te x N matrix of low rank plus noise, whose noise eigenvalues follow the Marchenko-Pastur law.
 * Input: a float32 te-major stack (n_te, nz, ny, nx), an optional uint8 mask (nz, ny, nx).  A centre is a voxel whose
 * whole window lies inside the volume; it is processed when its own voxel is in the mask (NULL: all) and its G is finite.
 * Everything below is float64 with one rounding per operation in the order written, nothing fused:
 *   1. G_ij = sum over the window of x_i x_j (i <= j; samples cast first): along x in increasing offset from 0.0, those
 *      sums along y, those along z (dims = 3).
 *   2. Cyclic Jacobi from A = G, V = I, at most 16 sweeps.  Before a sweep off = sum_{p<q} A_pq^2 (row-major from 0.0); the
 *      centre stops when off == 0.0.  A sweep visits (p, q), p < q, row by row: g = |A_pq|; if |A_pp| + g == |A_pp| and
 *      |A_qq| + g == |A_qq| then A_pq = 0.0; if A_pq == 0.0 the pair is skipped; else theta = (A_qq - A_pp) / (2 A_pq),
 *      t = sgn(theta) / (|theta| + sqrt(theta theta + 1)) with sgn(0) = +1, c = 1 / sqrt(t t + 1), s = t c; for k != p, q:
 *      A_kp' = c A_kp - s A_kq, A_kq' = s A_kp + c A_kq; A_pp -= t A_pq, A_qq += t A_pq, A_pq = 0; columns p and q of V get
 *      the same rotation.
 *   3. The eigenvalues (the diagonal) in ascending order s_0 .. s_{M-1}, ties by index.
 *   4. q = N, lam_r = max(s_0, 0) / q, clam = 0, cut = 0, sigma^2 = 0; for p = 0 .. M-1: lam = max(s_p, 0) / q, clam += lam,
 *      gamma = (p+1) / (q - (M-p-1)) (estimator 2) or (p+1) / q (estimator 1), a = clam / (p+1),
 *      b = (lam - lam_r) / (4 sqrt(gamma)); if b < a: sigma^2 = a, cut = p + 1.  The M - cut largest components are kept.
 *   5. P = sum of v_j v_j^T over the kept components in ascending order from 0.0; P = 0 at an unprocessed centre.
 *   6. For every voxel v: Pbar(v) = the ordered window sum of step 1 over the field of P (zero where there is no centre),
 *      cnt(v) = the number of processed centres whose window holds v,
 *      out_i(v) = float32((sum_j Pbar_ij(v) x_j(v), j ascending from 0.0) / cnt); the input sample when cnt = 0.
 *   7. sigma(v) = float32(sqrt(sigma^2)) and rank(v) = uint8(M - cut) of the centre clamp(v, radius, n - 1 - radius) (per
 *      windowed axis); 0 when that centre is unprocessed.
 * The noise is treated as Gaussian: at low SNR the Rician floor of magnitude data biases sigma low.
 * fetal_t2mapping_amd/_mppca.py states all of it in numpy; the device output is bit-identical to it. */
#define T2FIT_MPPCA_MAX_TE 16    /* n_te outside 2 .. this is refused; 2 .. 8 run register-resident kernels, 9 .. 16 a generic one */
#define T2FIT_MPPCA_MAX_RADIUS 4 /* radius outside 1 .. this is refused */

typedef struct t2fit_mppca_params {
  int32_t radius;    /* 1 .. T2FIT_MPPCA_MAX_RADIUS; default 2 */
  int32_t dims;      /* 2: the window spans x, y (every slice on its own, default); 3: x, y, z */
  int32_t estimator; /* 1 or 2 (default): gamma of step 4 */
  int32_t flags;     /* must be 0 */
} t2fit_mppca_params;

int t2fit_mppca_params_default(t2fit_mppca_params *p);

/* Bytes of the workspace of a denoising call (out_dev != NULL); plain arithmetic, no device.  With up() rounding up to
 * 256 and centres = (nz or nz - 2 radius) (ny - 2 radius) (nx - 2 radius):
 *   up(8 * n_te (n_te + 1) / 2 * centres)  [the projector field, pair-major]  +  up(centres)  [processed flags]
 * Refuses what t2fit_mppca_dev refuses in p and the sizes. */
int t2fit_mppca_workspace_bytes(const t2fit_mppca_params *p, int n_te, int nz, int ny, int nx, size_t *bytes);

/* mask_dev, out_dev, sigma_dev (float32, nz ny nx), rank_dev (uint8, nz ny nx) may each be NULL, the three outputs not all
 * at once.  out_dev == NULL is the estimate-only call: one kernel, no projector field, and workspace_dev may be NULL with
 * workspace_bytes 0.  Otherwise the workspace is aligned to 256 bytes, of any content, and two kernels run.  out_dev may
 * equal in_dev; sigma_dev and rank_dev must not overlap in_dev.  Asynchronous on `stream`; no allocation, copy or
 * synchronisation inside.  Every argument is checked before HIP is touched and a refusal (T2FIT_E_INVALID) leaves a
 * message: p NULL, dims, radius, estimator, flags, n_te outside 2 .. T2FIT_MPPCA_MAX_TE, a window that holds no more voxels
 * than there are echoes, a windowed axis shorter than 2 radius + 1, in_dev NULL, float pointers not aligned to 4 bytes,
 * a missing, misaligned or short workspace. */
int t2fit_mppca_dev(const t2fit_mppca_params *p, const float *in_dev, const uint8_t *mask_dev, float *out_dev, float *sigma_dev,
                    uint8_t *rank_dev, int n_te, int nz, int ny, int nx, void *workspace_dev, size_t workspace_bytes, void *stream);

/* ---- Atlas-prior EM tissue segmentation (additive to ABI 5) ---------------------------------------------------------
 * A Gaussian mixture over C channels (echoes of one subject) and K classes with spatial priors and a mean-field Potts
 * term (Van Leemput 1999; Habas 2010 for fetal brains).  The library provides the steps; the loop, the class model
 * (means, precisions, log-determinants from the sums) and the stop rule are host code, fetal_t2mapping_amd/_seg.py, which
 * also states every step below in numpy.  Volumes are (nz, ny, nx), x fastest; p, pi and the priors are K planes, y is C
 * planes, float32; masks are uint8.  M is the set of voxels with mask != 0 and every channel finite: t2fit_seg_mask_dev
 * writes it as 0 / 1, and the mask_dev of the other steps must be such a mask (they test their own voxel's channels again,
 * but trust the mask for its neighbours).  Everything is float64 with one rounding per operation in the order written,
 * nothing fused, and one rounding to float32 where a float32 is stored:
 *   priors     plane k = the image labels == classes[k] (1.0 / 0.0), blurred along x, then y, then z; a pass is
 *              float32(sum_j w_j (double)in[i + j - r], j = 0 .. 2 r ascending from 0.0, taps beyond the volume left out).
 *   normalise  pi_ik = float32(((double)prior_ik + floor) / ((sum_l (double)prior_il, l ascending from 0.0) + K floor)) in
 *              mask != 0, +0.0 outside.
 *   sums       per class k, M = 1 + C + C (C + 1) / 2 values: S0 = sum p, S1_c = sum p y_c, S2_cd = sum (p y_c) y_d (c <= d,
 *              row-major), over the voxels of M.  The tree: workgroup b takes the voxels 1024 b .. 1024 b + 1023 of the flat
 *              volume; its lane t (0 .. 255) adds the terms of the voxels 1024 b + 256 j + t, j = 0 .. 3 in this order from
 *              0.0, leaving out those beyond the volume or outside M; each wave of 64 lanes folds by v = v + v[lane ^ s] for
 *              s = 32, 16, 8, 4, 2, 1; the four waves add as ((w0 + w1) + w2) + w3.  The workgroup values are then folded in
 *              passes until one is left (at least one pass): a pass turns 256 consecutive values (zeros beyond the end)
 *              into one by s[t] = s[t] + s[t + h] for t < h, h = 128, 64, .. 1.  sums_out[k M + m].
 *   estep      for a voxel of M and a live class k, with model[k] = (mu_c (C), the upper triangle of the precision P_cd
 *              row-major, c_k): t_c = (double)y_c - mu_c; d = sum over c <= d row-major from 0.0 of
 *              (((c == d ? 1 : 2) P_cd) t_c) t_d; n = sum from 0.0 of (1 - (double)p_old_jk) over the neighbours j inside the
 *              volume with mask != 0, in the order -z, -y, -x, +x, +y, +z; a_k = (c_k - 0.5 d) - beta n; m = max a_k;
 *              q_k = (double)pi_ik exp(a_k - m); s = sum of q_k, k ascending from 0.0; p_new_ik = float32(q_k / s).  A class
 *              that is not live and a voxel outside M get +0.0.  (exp is the device library's: the statement's differs in
 *              the last bits, so this step is within 1 float32 ulp of it, not bit-identical.)
 *   labels     classes[the first k of the largest p_ik] where mask != 0, 0 elsewhere.
 * All entry points are asynchronous on `stream`, allocate nothing and check every argument before HIP is touched; a
 * refusal (T2FIT_E_INVALID) leaves a message that names the argument: n_class outside 2 .. T2FIT_SEG_MAX_CLASSES, n_chan
 * outside 1 .. T2FIT_SEG_MAX_CHANNELS, a radius outside 0 .. T2FIT_SEG_MAX_RADIUS, sizes < 1 or a volume above 2^37 voxels,
 * NULL pointers, float pointers not aligned to 4 bytes (double ones to 8), floor or beta negative or not finite,
 * p_new_dev == p_old_dev, no live class. */
#define T2FIT_SEG_MAX_CLASSES 8
#define T2FIT_SEG_MAX_CHANNELS 4
#define T2FIT_SEG_MAX_RADIUS 32

/* Bytes of the workspace that serves both t2fit_seg_priors_dev and t2fit_seg_sums_dev; plain arithmetic, no device.  With
 * up() rounding up to 256, n = nz ny nx, b = ceil(n / 1024) and Q = n_class (1 + n_chan + n_chan (n_chan + 1) / 2):
 *   max(up(4 n_class n)  [the y pass of the blur],  up(8 Q b) + up(8 Q ceil(b / 256))  [the partial sums, two buffers]) */
int t2fit_seg_workspace_bytes(int n_class, int n_chan, int nz, int ny, int nx, size_t *bytes);

/* m_out = 1 where mask_dev != 0 (NULL: everywhere) and all n_chan channels of y_dev are finite, else 0. */
int t2fit_seg_mask_dev(const float *y_dev, const uint8_t *mask_dev, int n_chan, int64_t n_vox, uint8_t *m_out_dev, void *stream);

/* classes and the taps (2 r + 1 doubles per axis, host memory) are read before the call returns.  The workspace (of any
 * content, aligned to 4 bytes) must not overlap prior_out_dev. */
int t2fit_seg_priors_dev(const int32_t *labels_dev, const int32_t *classes, int n_class, int nz, int ny, int nx, const double *taps_z,
                         int rz, const double *taps_y, int ry, const double *taps_x, int rx, float *prior_out_dev, void *workspace_dev,
                         void *stream);

/* pi_out_dev must not overlap prior_dev. */
int t2fit_seg_normalise_dev(const float *prior_dev, const uint8_t *mask_dev, int n_class, int64_t n_vox, double floor, float *pi_out_dev,
                            void *stream);

/* Writes n_class (1 + n_chan + n_chan (n_chan + 1) / 2) doubles to sums_out_dev (device memory).  The workspace is of any
 * content and aligned to 8 bytes. */
int t2fit_seg_sums_dev(const float *p_dev, const float *y_dev, const uint8_t *mask_dev, int n_class, int n_chan, int nz, int ny, int nx,
                       double *sums_out_dev, void *workspace_dev, void *stream);

/* model: n_class rows of n_chan + n_chan (n_chan + 1) / 2 + 1 doubles, live: n_class flags, both host memory, read before
 * the call returns (they travel in the kernel's arguments). */
int t2fit_seg_estep_dev(const float *p_old_dev, const float *pi_dev, const float *y_dev, const uint8_t *mask_dev, const double *model,
                        const int32_t *live, double beta, int n_class, int n_chan, int nz, int ny, int nx, float *p_new_dev, void *stream);

int t2fit_seg_labels_dev(const float *p_dev, const uint8_t *mask_dev, const int32_t *classes, int n_class, int64_t n_vox,
                         int32_t *labels_out_dev, void *stream);

/* ---- Orthogonal-stack reconstruction: resample to an isotropic grid and merge -------------------------------------
 * Steps 1 and 2 of the reference's run_qmri_reconstruction.py: every acquired thick-slice stack (ax / cor / sag, one per
 * echo time) is resampled to a 1 mm grid with linear interpolation (utils/qmri_utils.py resample_volume, :62-80), the
 * two moving ones are resampled onto the fixed one's grid after a rigid registration, and the three are averaged
 * (reconstruct_vol_trilinear, :82-136).  Rigid transforms enter through the affines below (identity = the reference's
 * "no motion" reading); the registration that finds them is further down (t2fit_register_sums_dev).  fetal_t2mapping_amd/_resample.py restates
 * everything here in numpy, geometry included; the device output is bit-identical to it and the same from call to call.
 *
 * Volumes are (nz, ny, nx) with x fastest.  Geometry stays on the host: a stage is described by 12 doubles A (row-major
 * 3 x 4), the continuous source index of the integer output index (ix, iy, iz),
 *   c_a = ((A[4a] ix + A[4a+1] iy) + A[4a+2] iz) + A[4a+3]      a = 0 (x), 1 (y), 2 (z), float64, no fused multiply-add.
 * The voxel is inside iff -0.5 <= c_a < n_a - 0.5 on all three axes; otherwise the result is default_value.
 * T2FIT_INTERP_LINEAR: b_a = clamp(floor(c_a), 0, n_a - 1), d_a = max(c_a - b_a, 0), upper neighbour min(b_a + 1, n_a - 1)
 * (the half-voxel rim replicates the edge); interpolation along x, then y, then z in float64 as lo + d (hi - lo); where
 * d_a == 0 the upper sample along a is not read and the result is lo (a resample onto the source's own nodes is the
 * identity bit for bit, and an Inf next to a node does not become a NaN); where lo + d (hi - lo) is NaN (an infinite lo:
 * Inf - Inf) the level is lo + hi, so a voxel whose nodes of non-zero weight hold an Inf is that Inf, and NaN only if they
 * hold a NaN or both Infs; one rounding to float32 at the end.  With
 * T2FIT_RESAMPLE_INTEGER_CAST the float64 result is first truncated toward zero and clamped to [-32768, 32767] (a stack
 * that is int16 on disk and keeps its pixel type through sitk.Resample).
 * T2FIT_INTERP_NEAREST: the node floor(c_a + 0.5), clamped into the volume, is copied (float32 or int32 sources).
 * Parity with ITK on the rim, on nearest-neighbour ties and on the integer cast is not pinned. */
#define T2FIT_INTERP_LINEAR 0
#define T2FIT_INTERP_NEAREST 1
#define T2FIT_RESAMPLE_F32 0
#define T2FIT_RESAMPLE_I32 1
#define T2FIT_RESAMPLE_INTEGER_CAST 1 /* flags bit of t2fit_resample_dev and t2fit_reconstruct_dev */
#define T2FIT_RECON_CHAIN 2           /* flags bit of t2fit_reconstruct_*: the chain of single stages, not the fused kernel */

/* One stage: n_vol volumes of (nz, ny, nx) at src_dev (src_type T2FIT_RESAMPLE_F32, or T2FIT_RESAMPLE_I32 with
 * T2FIT_INTERP_NEAREST), which share the geometry (the echoes of one orientation), into n_vol volumes of (oz, oy, ox) of
 * the same type at out_dev.  default_value is rounded to the volume's type.  The workgroups walk their output bricks
 * along the output axis with the largest |A[0..2]| (the one that follows the source's x), so that the reads are
 * contiguous whichever way the stack is oriented; the result does not depend on it.  Asynchronous on `stream`: one
 * launch, no allocation, copy or synchronisation.  Every argument is checked before HIP is touched (T2FIT_E_INVALID and
 * a message): NULL src_dev / out_dev / A, out_dev == src_dev, pointers not aligned to 4 bytes, unknown src_type or
 * interp, an int32 source with linear interpolation, flags other than T2FIT_RESAMPLE_INTEGER_CAST (which goes with
 * linear only), n_vol or a size < 1, more than 2^40 elements in a stack, more than 2^31-1 bricks of 512 output voxels,
 * a non-finite entry of A, a default_value outside int32 for an int32 source. */
int t2fit_resample_dev(const void *src_dev, int src_type, int nz, int ny, int nx, const double *A, void *out_dev, int oz, int oy,
                       int ox, int n_vol, int interp, double default_value, int flags, void *stream);

/* The whole reconstruction of n_vol echoes.  Index 0 is the fixed orientation, 1 and 2 the moving ones in the order of
 * ["ax", "cor", "sag"] without the fixed one.  lo_size[9] / hi_size[9]: (nz, ny, nx) of the three acquired stacks L_s and
 * of their isotropic grids H_s; A1[36]: the three stage-1 affines (H_s index -> L_s index); A2[24]: the two stage-2
 * affines (H_0 index -> H_m index, the rigid transform of moving stack m folded in).
 *   stage 1  H_s = linear resample of L_s by A1[s]                          s = 0, 1, 2, default 0
 *   stage 2  R_m = linear resample of H_m (float32) by A2[m - 1] onto H_0   m = 1, 2, default 0
 *   merge    out = ((H_0 + R_1) + R_2) / 3 in float64, rounded to float32   (np.mean of the three, as the reference)
 * T2FIT_RESAMPLE_INTEGER_CAST applies to both stages.  out_dev: float32 [n_vol][hi_size[0..2]], the layout
 * t2fit_tv_denoise_dev and t2fit_volume_dev (te-major) take.
 * flags = 0 runs one fused kernel: every stage-2 tap is a stage-1 sample formed on the spot and rounded to float32 as the
 * stored intermediate would be; no workspace (workspace_dev may be NULL).  T2FIT_RECON_CHAIN runs three stage-1 and two
 * stage-2 launches of the single-stage kernel plus a merge and needs
 *   t2fit_reconstruct_workspace_bytes = up(4 n_vol |H_1|) + up(4 n_vol |H_2|) + 2 up(4 n_vol |H_0|),  up(v) = v rounded up
 * to 256, aligned to 256 bytes.  Both forms give the same bytes; at 256^3 x 8 from three 1 x 1 x 4.5 mm stacks the chain
 * measured 3.5 ms and the fused kernel 4.6 ms, so the Python mirror asks for the chain.  Asynchronous on `stream`; no allocation, copy or
 * synchronisation.  Checked before HIP is touched: NULL stacks_dev (or an entry) / lo_size / hi_size / A1 / A2 / out_dev /
 * bytes, a stack that is out_dev, pointers not aligned to 4 bytes, undefined flags, n_vol or a size < 1, too many
 * elements or bricks (as above), non-finite affines, a workspace that is missing, too small or misaligned for the chain.
 * t2fit_reconstruct_workspace_bytes is plain arithmetic and needs no device. */
int t2fit_reconstruct_workspace_bytes(int n_vol, const int32_t *lo_size, const int32_t *hi_size, int flags, size_t *bytes);
int t2fit_reconstruct_dev(const float *const *stacks_dev, const int32_t *lo_size, const double *A1, const int32_t *hi_size,
                          const double *A2, float *out_dev, int n_vol, int flags, void *workspace_dev, size_t workspace_bytes,
                          void *stream);

/* ---- Super-resolution reconstruction: the acquisition operator of a thick-slice stack and its adjoint -------------------
 * The averaged merge above interpolates each stack to 1 mm and so keeps the blur of the slice thickness along three axes.
 * Here a thick slice is modelled as the slice-profile average of the 1 mm volume and that model is inverted, per echo,
 *   minimise over x:  1/2 sum_s ||A_s x - y_s||^2 + weight * TV(x)       (TV isotropic with forward differences)
 * by proximal gradient from the averaged merge, x <- prox(x - tau sum_s A_s^T (A_s x - y_s)).  The prox of tau weight TV
 * is t2fit_tv_denoise_dev with dims = 3, whose `weight` w stands for exactly one times TV (its fixed point minimises
 * 1/2 ||u - f||^2 + w TV(u)), so it is called with w = tau * weight, eps = 0 and max_iter = the prox iterations;
 * tau = 1 / sum_s max_v (A_s^T 1)[v] (the rows of A_s sum to 1, so ||A_s||^2 is at most its largest column sum).  The
 * loop is host code over the two entry points below (fetal_t2mapping_amd/_gpu_sr.py); fetal_t2mapping_amd/_sr.py restates
 * operator, adjoint and loop in numpy and the device results are bit-identical to it.  Additive to ABI 5.
 *
 * H is the high-resolution grid (hz, hy, hx), stack s a grid (lz, ly, lx), x fastest.  B (12 doubles, the index affine of
 * t2fit_resample_dev) maps an integer H index v to the continuous stack index u = c(B, v), the expression and rounding
 * order of c_a above.  The weight of the pair (sample j, voxel v) is separable in the stack's own axes,
 *   w(j, v) = (tri(u_x - j_x) * tri(u_y - j_y)) * prof(u_z - j_z),   tri(d) = max(0, 1 - |d|),
 * with thickness = slice thickness / slice spacing (> 0) and one of two polynomial profiles:
 *   T2FIT_SR_PROFILE_BOX       prof(d) = 1 for -h <= d < h, else 0, h = thickness / 2 (half-open: abutting slices
 *                              partition the axis)
 *   T2FIT_SR_PROFILE_BSPLINE3  prof(d) = beta3(|d| / a), a = thickness / 1.4447034489287527 (the cubic B-spline's full
 *                              width at half maximum, so the profile's is the thickness): with t = |d| / a,
 *                              (2/3 - t t) + 0.5 ((t t) t) for t < 1, ((q q) q) / 6 with q = 2 - t for t < 2, else 0.
 * Both directions form w from the very same u, so the operator and its adjoint hold the same bits.  In float64, one
 * rounding per operation as written, a pair of weight 0 skipped:
 *   N[j]         = sum_v w(j, v)                           v inside H, ascending (z, y, x)
 *   (A x)[j]     = (sum_v w(j, v) x[v]) / N[j]             same order; x widened to float64
 *   a sample counts iff N[j] > 0 and its mask byte (when a mask is given) is not 0
 *   r[j]         = (A x)[j] - y[j] if the sample counts (just (A x)[j] without y), else 0;  rounded to float32 once
 *   g[v]         = sum_s sum_j (w_s(j, v) r_s[j]) / N_s[j]   stacks in order, then the samples that count in ascending
 *                                                            (z, y, x), one accumulator
 *   out[v]       = g[v] (x_dev NULL), or x[v] - tau g[v];  rounded to float32 once
 * The forward kernel looks for its voxels in the box |v_a - floor(c(Binv, j)_a + 0.5)| <= radius[a]; the box only has to
 * cover the support, the result does not depend on it. */
#define T2FIT_SR_PROFILE_BOX 0
#define T2FIT_SR_PROFILE_BSPLINE3 1
#define T2FIT_SR_MAX_STACKS 6

/* Host arithmetic, no device: the inverse Binv[12] of B (by cofactors) and radius[3] (x, y, z) for supports of half-widths
 * half[3] (x, y, z) in stack-index units -- (1, 1, h) for the box, (1, 1, 2 a) for the B-spline:
 *   radius[a] = ceil(sum_b |Binv[4a + b]| half[b]) + 1
 * (the sum bounds the support around the exact preimage, 1/2 goes to the rounded centre, the rest to rounding).  Refuses
 * NULL pointers, non-finite entries, half-widths <= 0, a singular B (determinant 0 or a reach beyond 2^20 voxels). */
int t2fit_sr_plan_host(const double *B, const double *half, double *Binv, int32_t *radius);

/* Bytes of one buffer that holds what a loop over the two calls below keeps: up(4 n_vol |H|) for the update z plus, per
 * stack, up(8 |L_s|) for N_s and up(4 n_vol |L_s|) for r_s, up(v) = v rounded up to 256.  lo_size: (nz, ny, nx) per stack.
 * Plain arithmetic, no device; refuses n_stacks outside 1 .. T2FIT_SR_MAX_STACKS, sizes < 1 and more than 2^40 elements. */
int t2fit_sr_workspace_bytes(int n_stacks, const int32_t *lo_size, int hz, int hy, int hx, int n_vol, size_t *bytes);

/* One stack forward: out_dev [n_vol][lz][ly][lx] = r above from x_dev [n_vol][hz][hy][hx] and y_dev (same layout as
 * out_dev, or NULL for A x itself); mask_dev uint8 [lz][ly][lx] or NULL; N_dev float64 [lz][ly][lx] receives N, or NULL.
 * x_dev = out_dev = NULL with N_dev: the weights only.  One thread per sample walks its box once per chunk of 4 echoes.
 * Asynchronous on `stream`: one launch, no allocation, copy or synchronisation.  Checked before HIP is touched
 * (T2FIT_E_INVALID and a message): NULL B / Binv / radius, nothing to write, x_dev without out_dev or the reverse, n_vol or a
 * size < 1, more than 2^40 elements, non-finite B / Binv, a radius < 1, an unknown profile, thickness <= 0 or not finite,
 * float pointers not aligned to 4 bytes (N_dev: 8), out_dev == x_dev. */
int t2fit_sr_forward_dev(const float *x_dev, int hz, int hy, int hx, int n_vol, const double *B, const double *Binv,
                         const int32_t *radius, int profile, double thickness, const float *y_dev, const uint8_t *mask_dev, int lz,
                         int ly, int lx, float *out_dev, double *N_dev, void *stream);

/* All stacks back: out_dev [n_vol][hz][hy][hx] = g, or x - tau g with x_dev (out_dev == x_dev is allowed).  r_dev, N_dev,
 * mask_dev: HOST arrays of n_stacks device pointers (mask_dev or any of its entries may be NULL); lo_size 3, B 12, profile 1,
 * thickness 1 entries per stack.  N_dev[s] is what t2fit_sr_forward_dev wrote.  One thread per voxel, every stack in one
 * pass: 2 x 2 in-plane candidates times the floor(2 half-width) + 3 slices from floor(u_z - half-width) on.  Asynchronous on
 * `stream`: one launch.  Checked before HIP is touched: NULL pointers (x_dev and masks excepted), n_stacks outside 1 ..
 * T2FIT_SR_MAX_STACKS, sizes as above, non-finite B or tau, an unknown profile, thickness <= 0 or not finite, alignment as
 * above, a residual that is out_dev. */
int t2fit_sr_adjoint_dev(int n_stacks, const float *const *r_dev, const double *const *N_dev, const uint8_t *const *mask_dev,
                         const int32_t *lo_size, const double *B, const int32_t *profile, const double *thickness,
                         const float *x_dev, double tau, float *out_dev, int hz, int hy, int hx, int n_vol, void *stream);

/* ---- Super-resolution with a rigid pose per slice ---------------------------------------------------------------------
 * A stack acquired slice by slice from a moving subject is sharp within each slice, but every slice has its own pose.
 * Slice k of stack s then has its own index affine B[s][k] (12 doubles, H index -> continuous stack index) and the weight of
 * the pair (sample j = (j_x, j_y, j_z), voxel v) becomes
 *   w(j, v) = (tri(u_x - j_x) * tri(u_y - j_y)) * prof(u_z - j_z),     u = c(B[s][j_z], v)
 * Nothing else of the definition above changes: tri, both profiles and the half-open box, N[j] summed over v in ascending
 * (z, y, x) with zero weights skipped, the forward value (sum w x) / N - y, what "counts" means, float64 sums with one
 * rounding per operation and no atomics.  The adjoint's one accumulator per voxel runs over the stacks in order, within a
 * stack over ALL slices in ascending k (by index, not by position in space), and within a slice over the 2 x 2 in-plane
 * candidates (floor(u_y) + cy, floor(u_x) + cx) in ascending (cy, cx) with u from that slice's affine:
 *   acc += (w * r[j]) / N[j]   for the samples that count and have w > 0;   out = acc, or x - tau acc.
 * If every slice of a stack carries the stack's own affine, N, forward, adjoint and update are bit-identical to
 * t2fit_sr_forward_dev / t2fit_sr_adjoint_dev: the non-zero terms and their order are the same.
 * fetal_t2mapping_amd/_sr.py (forward_slices, adjoint_slices) restates both in numpy; same bits.  Additive to ABI 5.
 *
 * An affine per slice does not fit a kernel's argument segment, so the affines travel as a table in device memory: one
 * record of T2FIT_SR_SLICE_RECORD_BYTES = 208 bytes per slice, slice k at byte 208 k,
 *   bytes   0 ..  95   B[12]     float64, the slice's index affine
 *   bytes  96 .. 191   Binv[12]  float64, its inverse as t2fit_sr_plan_host forms it
 *   bytes 192 .. 203   radius[3] int32 (x, y, z), of t2fit_sr_plan_host for half-widths (1, 1, the profile's)
 *   bytes 204 .. 207   0
 * t2fit_sr_slice_table_host packs it on the host (no device; it validates every slice exactly as t2fit_sr_plan_host does
 * -- NULL, non-finite entries, a singular affine, a reach beyond 2^20 voxels -- before it writes a byte, and refuses
 * lz < 1, an unknown profile, a bad thickness and a buffer smaller than t2fit_sr_slice_table_bytes says); the caller
 * uploads the blob once and reuses it across the loop.  The table is data, not a trusted argument: whatever it holds, both
 * kernels terminate and stay inside their buffers (ranges are clamped to the grid; a non-finite centre or coordinate gives
 * an empty range). */
#define T2FIT_SR_SLICE_RECORD_BYTES 208
int t2fit_sr_slice_table_bytes(int lz, size_t *bytes);
int t2fit_sr_slice_table_host(int lz, const double *B /* [lz][12] */, int profile, double thickness, void *table_host,
                              size_t bytes);

/* t2fit_sr_forward_dev with table_dev (device memory, lz records, aligned to 8 bytes) in place of B / Binv / radius: sample
 * j walks the box of radii radius[j_z] around floor(c(Binv[j_z], j) + 0.5).  A workgroup lies inside one slice, so the
 * record is read once per wave.  Asynchronous on `stream`: one launch, no allocation, copy or synchronisation.  Checked
 * before HIP is touched: as t2fit_sr_forward_dev, and table_dev NULL or not aligned to 8 bytes. */
int t2fit_sr_slice_forward_dev(const float *x_dev, int hz, int hy, int hx, int n_vol, const void *table_dev, int profile,
                               double thickness, const float *y_dev, const uint8_t *mask_dev, int lz, int ly, int lx,
                               float *out_dev, double *N_dev, void *stream);

/* t2fit_sr_adjoint_dev with table_dev, a HOST array of n_stacks device pointers to the stacks' tables, in place of B.  A
 * workgroup owns a tile of 16 x 4 x 4 voxels.  Per stack, in passes of 256 slices, each lane bounds the tile's stack
 * coordinates under one slice's affine (interval arithmetic on the tile's index box, widened by 2^-40 of the terms'
 * magnitude for rounding) and keeps the slice iff the u_z bounds meet [k - half-width, k + half-width] and the u_x / u_y
 * bounds meet [-1, lx] / [-1, ly]; the survivors are listed in ascending k and every lane walks the list, forming the pair
 * weight from its own u.  The cull drops no slice that contributes and zero weights are skipped, so the result is the
 * definition's.  Any number of slices.  Asynchronous on `stream`: one launch.  Checked before HIP is touched: as
 * t2fit_sr_adjoint_dev, and a table pointer that is NULL or not aligned to 8 bytes. */
int t2fit_sr_slice_adjoint_dev(int n_stacks, const float *const *r_dev, const double *const *N_dev,
                               const uint8_t *const *mask_dev, const void *const *table_dev, const int32_t *lo_size,
                               const int32_t *profile, const double *thickness, const float *x_dev, double tau, float *out_dev,
                               int hz, int hy, int hx, int n_vol, void *stream);

/* ---- Outlier-robust super-resolution: slice weights and Huber sample weights ------------------------------------------
 * Single-shot stacks contain bad slices (signal drop-outs, spin-history stripes, slices registered to the wrong place) and
 * a plain least-squares data term writes them straight into the volume.  The robust loop minimises, per echo,
 *   1/2 sum_s sum_j omega_j (A_s x - y_s)_j^2 + weight * TV(x),     omega = q (per slice) * w (per sample) in [0, 1],
 * with omega recomputed from the current residuals at every iteration: the residuals r_s = A_s x - y_s of
 * t2fit_sr_forward_dev / t2fit_sr_slice_forward_dev are multiplied by omega in place before the adjoint, so A^T (omega r)
 * is the gradient of the weighted term; omega <= 1, so the step size tau stays valid.  Only +, *, /, sqrt and comparisons
 * appear, in float64 with one rounding per operation in the order written, so fetal_t2mapping_amd/_sr.py (robust_slice_sums,
 * robust_scale, robust_apply) states it in numpy to the same bits.  Additive to ABI 5.
 *
 * Every echo e on its own; the slices of all stacks are listed stack-major, ascending in slice index (n_slices = sum lz_s).
 *   counted   sample j of stack s is counted iff N_s[j] > 0, its mask byte (when there is a mask) is not 0, and r[e][j] is
 *             finite.
 *   sums      of slice k: c = the number of counted samples, q2 = sum (double)r * (double)r over them, in a fixed tree:
 *             thread t of 256 adds the samples i = t, t + 256, ... of the slice's ly lx in ascending i; a wave adds by the
 *             xor butterfly 32, 16, .., 1; the four waves meet as ((w0 + w1) + w2) + w3.  No atomics.
 *   scale     slice k is eligible iff c >= min_count, then m_k = q2 / c.  With v the n eligible m of the echo, sorted,
 *             sigma2 = max(0.5 (v[(n - 1) / 2] + v[n / 2]), sigma_floor^2).  n == 0 or sigma2 not > 0: robustness is off for
 *             the echo: every weight is 1, r stays bit for bit as it was (non-finite samples too) and sigma2 is reported 0.
 *   q_k       1 if the slice is not eligible or m_k <= T sigma2, else (T sigma2) / m_k,   T = slice_threshold^2
 *   w_j       1 if |r_j| <= delta, else delta / |r_j|,   delta = huber * sqrt(sigma2)
 *   apply     a counted sample becomes (float)((q_k w_j) (double)r_j), any other sample +0.0. */
#define T2FIT_SR_ROBUST_MAX_SLICES 4096
typedef struct t2fit_sr_robust_params {
  double slice_threshold; /* t > 0: a slice whose mean square residual exceeds t^2 sigma2 is weighted down */
  double huber;           /* h > 0: a sample beyond h sigma is weighted down */
  double sigma_floor;     /* >= 0: lower bound of sigma, in intensity units */
  int32_t min_count;      /* >= 1: counted samples a slice needs to take part in the scale and to be weighted */
  int32_t flags;          /* reserved, must be 0 */
} t2fit_sr_robust_params;

/* slice_threshold 1.5, huber 2.5, sigma_floor 0, min_count 16, flags 0 */
int t2fit_sr_robust_params_default(t2fit_sr_robust_params *p);

/* Bytes of one buffer that holds the three tables of t2fit_sr_robust_dev, in this order: up(16 n_vol n_slices) for the sums,
 * up(8 n_vol n_slices) for the slice weights, up(8 n_vol) for sigma2; up(v) = v rounded up to 256.  A loop carves it after
 * t2fit_sr_workspace_bytes, whose result does not change.  Plain arithmetic, no device; refuses what t2fit_sr_robust_dev
 * refuses in n_stacks, lo_size and n_vol. */
int t2fit_sr_robust_workspace_bytes(int n_stacks, const int32_t *lo_size, int n_vol, size_t *bytes);

/* The weighting above on the residuals of n_stacks stacks, in place.  r_dev, N_dev, mask_dev: HOST arrays of n_stacks
 * device pointers (r_dev[s] float32 [n_vol][lz][ly][lx], in / out; N_dev[s] float64 [lz][ly][lx] from t2fit_sr_forward_dev;
 * mask_dev or any of its entries may be NULL); lo_size: (lz, ly, lx) per stack.  Caller buffers on the device, float64:
 * sums_dev [n_vol][n_slices][2] = (c, q2), weights_dev [n_vol][n_slices] = q, sigma2_dev [n_vol].  Three launches are queued
 * on `stream` (the sums: a workgroup per slice and chunk of 4 echoes, N and the mask read once per chunk; the scale: a
 * workgroup per echo, ranks by counting in LDS; the apply: a thread per sample and chunk); no allocation, copy or
 * synchronisation.  Checked before HIP is touched (T2FIT_E_INVALID and a message): a NULL pointer (mask_dev and its entries
 * excepted), n_stacks outside 1 .. T2FIT_SR_MAX_STACKS, n_vol or a size < 1, a stack of more than 2^40 elements, more than
 * T2FIT_SR_ROBUST_MAX_SLICES slices in total, slice_threshold or huber not finite or not > 0, min_count < 1, sigma_floor
 * negative or not finite, flags != 0, a residual not aligned to 4 bytes, N or a table not aligned to 8. */
int t2fit_sr_robust_dev(int n_stacks, float *const *r_dev, const double *const *N_dev, const uint8_t *const *mask_dev,
                        const int32_t *lo_size, int n_vol, const t2fit_sr_robust_params *params, double *sums_dev,
                        double *weights_dev, double *sigma2_dev, void *stream);

/* ---- Masks and phantom labels: binary morphology, hole filling, seed labels, relabelling ------------------------------
 * What the reference builds on the host before a fit can start (utils/qmri_utils.py): build_mask (:223-252),
 * build_phantom_masks (:591-623), build_phantom_labels_v2 (:868-933), build_mask_from_labels (:935-951) and the lookup of
 * convert_synthseg_to_feta (:976-1009).  Additive to ABI 5: six new symbols (look them up to detect them).
 * fetal_t2mapping_amd/_morph.py restates every definition in numpy; the device results equal it, and
 * scipy.ndimage, bit for bit.  Parity with ITK's ball voxelisation is not pinned.
 *
 * Volumes are (nz, ny, nx) with x fastest; masks are uint8 (0 / not 0 in, 0 / 1 out).  Inside, a mask is bit-packed in the
 * workspace, 64 x voxels per word.  A structuring element is its footprint's sizes size[3] = (sz, sy, sx), each odd and
 * at most 65 (radius 32; the origin is the centre), and a run list of n_runs (1..16900) rows of four int32
 * (dz, dy, x0, x1): "the offsets (dz, dy, x), x0 <= x <= x1, belong to the element"; several runs per (dz, dy) row are
 * allowed, every run lies inside the footprint.  `size` and `runs` are HOST pointers.
 *   dilate  out[v] = OR  over s in S of in[v - s]     a voxel outside the volume reads as border_value
 *   erode   out[v] = AND over s in S of in[v + s]     (the exact dual: complement, reflected S, complemented border)
 *   close   `iterations` dilations, then as many erosions;  open: erosions, then dilations  (each with border_value:
 *           scipy's binary_closing / binary_opening)
 *   T2FIT_MORPH_UNBOUNDED (close / open, border_value 0): the operation on the unbounded domain -- the volume is extended
 *           by zeros as far as the element reaches (radius * iterations), what the dilation spills outside is kept for
 *           the erosion, and the result is cropped: ITK's safe border. */
#define T2FIT_MORPH_DILATE 0
#define T2FIT_MORPH_ERODE 1
#define T2FIT_MORPH_CLOSE 2
#define T2FIT_MORPH_OPEN 3
#define T2FIT_MORPH_UNBOUNDED 1 /* flags bit of t2fit_binary_morph_dev */
#define T2FIT_MORPH_F32 0       /* element types of t2fit_binary_threshold_dev / t2fit_seed_labels_dev */
#define T2FIT_MORPH_I32 1
#define T2FIT_MORPH_U8 2

/* Bytes of the workspace the calls below need for an (nz, ny, nx) volume; plain arithmetic, no device.  `reach`: 0, or
 * for T2FIT_MORPH_UNBOUNDED the largest radius * iterations that will be asked for (0..256).  With up(v) = v rounded up
 * to 256, P = up(8 (nz + 2 reach)(ny + 2 reach) ceil((nx + 2 reach) / 64)) the bytes of a packed grid:
 *   up(16 * 16900) [runs] + up(16 * 65 * 65) [element bitmap] + up(16 * 4096) [seeds] + 256 [flags] + 3 P
 * Refuses a size < 1 and a packed grid of 2^31 words or more. */
int t2fit_morph_workspace_bytes(int nz, int ny, int nx, int reach, size_t *bytes);

/* out[v] = (lo <= src[v] <= hi) as uint8 0 / 1; src_type T2FIT_MORPH_F32 or T2FIT_MORPH_I32; the comparison is made in
 * float64 (exact for both), a NaN gives 0; lo = -inf / hi = +inf leave a side open.  n_vox in 1..2^39-1.  Asynchronous on
 * `stream`; NULL pointers, a bad type or size, a NaN bound are T2FIT_E_INVALID before HIP is touched. */
int t2fit_binary_threshold_dev(const void *src_dev, int src_type, int64_t n_vox, double lo, double hi, uint8_t *out_dev,
                               void *stream);

/* op in T2FIT_MORPH_DILATE / ERODE / CLOSE / OPEN on in_dev into out_dev (device uint8 [nz ny nx]; out_dev == in_dev is
 * allowed: the input is packed before anything is written).  iterations in 1..8.  workspace_dev: at least
 * t2fit_morph_workspace_bytes bytes, aligned to 256.  The run list is copied to the device and the call returns when it
 * has been read (it waits for `stream` once, before its kernels are queued); the kernels are asynchronous on `stream`.
 * Checked before HIP is touched (T2FIT_E_INVALID and a message): NULL in_dev / out_dev / size / runs / workspace_dev, an
 * unknown op, a size < 1, an even or too large footprint (radius > 32), n_runs outside 1..16900, a run that is empty or
 * leaves the footprint, iterations outside 1..8, border_value not 0 / 1, undefined flags, T2FIT_MORPH_UNBOUNDED with
 * dilate / erode or border_value 1, a workspace that is too small or misaligned. */
int t2fit_binary_morph_dev(int op, const uint8_t *in_dev, uint8_t *out_dev, int nz, int ny, int nx, const int32_t *size,
                           const int32_t *runs, int n_runs, int iterations, int border_value, int flags, void *workspace_dev,
                           size_t workspace_bytes, void *stream);

/* out = in plus its holes: the background is flooded from the volume's border through faces (scipy's default structure,
 * ITK's fullyConnected = false) and the output is the complement of what was reached.  slice_axis = -1: one 3-D problem;
 * 0, 1, 2: every plane perpendicular to that axis of the (z, y, x) array is its own 2-D problem whose border is the
 * plane's rim (build_mask: 2, planes of (z, y)).  Tiles of 8 x 8 x 256 voxels are grown to their fixed point on chip and
 * swept until a sweep changes nothing; the reached set only grows and its fixed point is unique, so the result -- and
 * the sweep count -- is a function of the input alone and there is no iteration cap.
 * THIS CALL SYNCHRONISES `stream`: the host reads the sweeps' flags back from pinned memory every four sweeps.  Only the
 * final unpack is still in flight on return.  *n_sweeps_out (HOST pointer, or NULL): sweeps run, the last of which
 * changed nothing.  out_dev == in_dev is allowed.  Checked before HIP is touched: NULL in_dev / out_dev / workspace_dev,
 * a size < 1, slice_axis outside -1..2, a workspace that is too small or misaligned. */
int t2fit_fill_holes_dev(const uint8_t *in_dev, uint8_t *out_dev, int nz, int ny, int nx, int slice_axis, void *workspace_dev,
                         size_t workspace_bytes, int32_t *n_sweeps_out, void *stream);

/* out[v] = max over the seeds s of labels[s] * [v - seed_s in S], 0 where no seed reaches: a ball painted at every seed,
 * merged with a maximum (build_phantom_labels_v2).  seeds: HOST int32 [n_seeds][3] = (x, y, z) indices as the reference
 * indexes an image (a seed may lie outside the volume; what leaves the volume is clipped); labels: HOST int32 [n_seeds],
 * >= 0 and <= 255 for a uint8 output; n_seeds in 1..4096.  out_type T2FIT_MORPH_U8 or T2FIT_MORPH_I32.  The seeds and the
 * element are copied to the workspace and the call returns when they have been read (it waits for `stream` once); the
 * kernel is asynchronous.  Checked before HIP is touched, as t2fit_binary_morph_dev. */
int t2fit_seed_labels_dev(const int32_t *seeds, const int32_t *labels, int n_seeds, const int32_t *size, const int32_t *runs,
                          int n_runs, int nz, int ny, int nx, void *out_dev, int out_type, void *workspace_dev,
                          size_t workspace_bytes, void *stream);

/* out[v] = lut[in[v]] where 0 <= in[v] < n_lut, else 0 (int32 -> int32, all device pointers; out_dev == in_dev is
 * allowed).  n_vox in 1..2^39-1.  Asynchronous on `stream`. */
int t2fit_relabel_dev(const int32_t *in_dev, int64_t n_vox, const int32_t *lut_dev, int n_lut, int32_t *out_dev, void *stream);

/* ---- Connected components: labels, sizes, boxes, centroid sums, selection tables -------------------------------------------
 * No reference counterpart (the reference never asks which voxels belong together); the definition is
 * scipy.ndimage.label's.  Additive to ABI 5: four new symbols (look them up to detect them).
 * fetal_t2mapping_amd/_components.py states every result in numpy; all of it is integer arithmetic and the device
 * results equal the statement in every element.
 *
 * A volume is (nz, ny, nx) with x fastest and fewer than 2^31 voxels; v = (z ny + y) nx + x is a voxel's linear index.
 * Input T2FIT_MORPH_U8: foreground = not 0.  Input T2FIT_MORPH_I32: classes -- two voxels are connected only when they
 * are neighbours AND hold the same value, which is not 0 (one labelling of a whole multi-class volume).  connectivity
 * 1, 2, 3: the 6, 18, 26 neighbours that differ in at most that many coordinates (scipy's
 * generate_binary_structure(3, connectivity)); a 2-D problem is a volume with nz = 1.  Labels: int32, 0 on the
 * background, 1..n on the components, numbered in ascending order of each component's smallest linear index (scipy's
 * numbering).
 *
 * The labelling is a lock-free union-find in which a parent is never larger than its child: tiles of
 * T2FIT_COMPONENTS_TILE_Z x _Y x _X voxels are solved in LDS, the tile faces are merged with atomic minima, the trees
 * are flattened and the roots ranked by a fixed prefix sum.  No wave waits for another and every loop is bounded, so
 * the result does not depend on how the device schedules the work. */
#define T2FIT_COMPONENTS_TILE_Z 4
#define T2FIT_COMPONENTS_TILE_Y 8
#define T2FIT_COMPONENTS_TILE_X 64

/* Bytes of the workspace of t2fit_components_label_dev; plain arithmetic, no device.  With up(v) = v rounded up to 256:
 *   256 [the count] + up(4 ceil(nz ny nx / 1024)) [roots per 1024 voxels]
 * Refuses a size < 1 and a volume of 2^31 voxels or more. */
int t2fit_components_workspace_bytes(int nz, int ny, int nx, size_t *bytes);

/* in_dev (device uint8 or int32 [nz ny nx], in_type T2FIT_MORPH_U8 or T2FIT_MORPH_I32) -> labels_dev (device int32
 * [nz ny nx], not the input; it serves as the parent array on the way).  Seven launches on `stream`, asynchronous.  The
 * number of components n is left in the first int32 of the workspace; with n_out (HOST pointer, may be NULL) the call
 * also waits for `stream` once and returns n there, through pinned memory.  Checked before HIP is touched
 * (T2FIT_E_INVALID and a message): NULL in_dev / labels_dev / workspace_dev, an unknown in_type, a size < 1, 2^31 voxels
 * or more, a connectivity outside 1..3, an int32 volume not aligned to 4 bytes, labels_dev == in_dev, a workspace that
 * is too small or not aligned to 256 bytes. */
int t2fit_components_label_dev(const void *in_dev, int in_type, int nz, int ny, int nx, int connectivity, int32_t *labels_dev,
                               int32_t *n_out, void *workspace_dev, size_t workspace_bytes, void *stream);

/* Per value i = 0..n of an int32 label volume (other values are ignored; row 0 is the background), n + 1 rows each:
 *   sizes_dev int64 [n + 1]       the number of voxels
 *   bbox_dev  int32 [n + 1][6]    (z0, y0, x0, z1, y1, x1), inclusive; of a value that does not occur (nz, ny, nx, -1, -1, -1)
 *   sums_dev  int64 [n + 1][3]    (sum of z, sum of y, sum of x): the centroid times the size
 * Any of the three may be NULL.  Integers, hence exact in any order: one pass with 64-bit atomics; the lanes of a wave
 * that hold the same value combine first.  Asynchronous on `stream`.  Refused before HIP is touched: NULL labels_dev, a
 * size < 1, 2^31 voxels or more, n < 0, a misaligned pointer. */
int t2fit_components_stats_dev(const int32_t *labels_dev, int nz, int ny, int nx, int n, int64_t *sizes_dev, int32_t *bbox_dev,
                               int64_t *sums_dev, void *stream);

/* The selection table lut_dev (device int32 [n + 1], lut[0] = 0) for t2fit_relabel_dev, from sizes_dev (device int64
 * [n + 1], row 0 ignored).  Component i passes when min_size <= size[i] and (max_size == 0 or size[i] <= max_size).
 * largest = 0: what passes is kept.  largest = 1: of what passes only the largest is kept, on a tie the lowest label (the sizes
 * of t2fit_components_stats_dev lie in 0..2^31-1; `largest` compares a size outside 0..2^32-1 as clamped to that range).
 * renumber = 0: a kept component maps to its own label; renumber = 1: to its rank (1..) among the kept.  What is not
 * kept maps to 0.  *n_kept_out (HOST pointer, or NULL): the number kept; the call then waits for `stream` once.  The
 * temporaries live in the library's per-stream scratch.  Refused before HIP is touched: NULL sizes_dev / lut_dev, n < 0,
 * min_size < 0, max_size < 0, largest or renumber other than 0 / 1, a misaligned pointer. */
int t2fit_components_lut_dev(const int64_t *sizes_dev, int n, int64_t min_size, int64_t max_size, int largest, int renumber,
                             int32_t *lut_dev, int32_t *n_kept_out, void *stream);

/* ---- Exact Euclidean distance transform: squared distances and nearest sites -----------------------------------------------
 * No reference counterpart; the distances are scipy.ndimage.distance_transform_edt's.  Additive to ABI 5: three new
 * symbols (look them up to detect them).  fetal_t2mapping_amd/_edt.py states every result in numpy and the device
 * results equal the statement in every bit of d2 (inf included) and every index.
 *
 * A volume is (nz, ny, nx) with x fastest, each axis in 1..T2FIT_EDT_MAX_AXIS and fewer than 2^31 voxels;
 * v = (z ny + y) nx + x is a voxel's linear index.  The sites are the voxels equal to 0 (invert = 1, scipy's convention
 * for a mask) or not equal to 0 (invert = 0).  spacing = (sz, sy, sx).  The definition is three passes in the order z, y, x:
 *   start:   g = 0.0 at a site, +inf elsewhere; key = the site's linear index, -1 elsewhere
 *   pass a:  g'[i] = min over j along axis a of g[j] + t t, t = (double)(i - j) s_a (a multiply, a square, an add);
 *            key'[i] = key[j] of the minimising j, among equal values the LOWEST key; a j with key -1 never wins
 * so d2 = ((dz sz)^2 + (dy sy)^2) + (dx sx)^2 of the nearest site, exact for unit and dyadic spacing, and index is the
 * lowest linear index among the nearest sites where the arithmetic is exact.  With no site: d2 = +inf, index = -1.
 * (Spacings whose squares overflow or underflow a double are outside this guarantee.) */
#define T2FIT_EDT_MAX_AXIS 2048

/* Bytes of the workspace of t2fit_edt_dev; plain arithmetic, no device.  With up(v) = v rounded up to 256 and
 * n = nz ny nx:   2 up(8 n) [g of two passes] + 2 up(4 n) [their keys]
 * Refuses an axis outside 1..T2FIT_EDT_MAX_AXIS and a volume of 2^31 voxels or more. */
int t2fit_edt_workspace_bytes(int nz, int ny, int nx, size_t *bytes);

/* vol_dev (device uint8 [nz ny nx]) -> d2_dev (device double [nz ny nx], may be NULL) and index_dev (device int32
 * [nz ny nx], may be NULL; not both).  spacing: HOST pointer to 3 doubles, NULL = 1.  Three launches on `stream`,
 * asynchronous: the z pass sweeps each column twice, the y pass scans outward through L2, the x pass scans outward over
 * rows staged in LDS; the work of a scan is proportional to the distance found.  Refused before HIP is touched
 * (T2FIT_E_INVALID and a message, nothing launched): NULL vol_dev, both outputs NULL, invert not 0 / 1, an axis out of
 * range, 2^31 voxels or more, a spacing that is not finite or <= 0, a misaligned d2_dev / index_dev, a NULL, misaligned
 * (256 bytes) or too small workspace. */
int t2fit_edt_dev(const uint8_t *vol_dev, int invert, int nz, int ny, int nx, const double *spacing, double *d2_dev, int32_t *index_dev,
                  void *workspace_dev, size_t workspace_bytes, void *stream);

/* out[v] = labels[index[v]] where where[v] != 0 and 0 <= index[v] < n, else labels[v] (v in 0..n-1; an index outside
 * the volume counts as no site).  All device pointers; out_dev must not be labels_dev.  n in 1..2^31-1.  One launch,
 * asynchronous.  Refused before HIP is touched: a NULL pointer, n out of range, an int32 buffer not aligned to 4 bytes,
 * out_dev == labels_dev. */
int t2fit_edt_fill_dev(const int32_t *labels_dev, const uint8_t *where_dev, const int32_t *index_dev, int64_t n, int32_t *out_dev,
                       void *stream);

/* ---- Rigid registration: the correlation metric's sums and the pyramid levels -------------------------------------------
 * The device half of a rigid registration built from the ingredients of the reference's registration_itk
 * (utils/qmri_utils.py:167-221): correlation metric, fixed and moving masks, linear interpolator.  The metric's
 * arithmetic, the Euler transform and the regular-step gradient descent are host code
 * (fetal_t2mapping_amd/_register.py, which also restates everything here in numpy; the device results equal it bit for
 * bit).  Parity with elastix, which the reference calls, is not pinned.  Additive to ABI 5: four new
 * symbols (look them up to detect them).
 *
 * A is the index affine of t2fit_resample_dev: 12 doubles, fixed index (ix, iy, iz) -> continuous moving index c, in the
 * order of evaluation written there.  A fixed voxel COUNTS iff fixed_mask != 0, c passes the inside test
 * (-0.5 <= c_a < n_a - 0.5 on all axes) and the moving mask at the nearest node floor(c_a + 0.5), clamped, is != 0.  For
 * a voxel that counts: f = the fixed sample; m = the float64 interpolant of T2FIT_INTERP_LINEAR (clamped lower node,
 * replicated upper node on the rim, x then y then z as lo + d (hi - lo), a zero weight returns lo), not rounded to
 * float32; g_a = dm/dc_a = the difference of the two neighbours along a, interpolated along the other two axes with the
 * same weights and rule, and 0 where m is flat along a (the upper neighbour is the clamped lower one, or c_a < 0).
 * sums[43], float64:
 *   [0] N  [1] sum f  [2] sum m  [3] sum f f  [4] sum m m  [5] sum f m
 *   [6 + 4 (3 w + a) + j] sum (w g_a) u_j     w in (1, f, m), a in (x, y, z), u = (ix, iy, iz, 1)
 *   [42] reserved: +0.0 (N, the 5 moments and the 36 gradient sums are 42 numbers; the array keeps 43 slots)
 * Every product rounds once (w g_a first, then u_j; u_3 = 1 is no multiplication), no fused multiply-add; a voxel that
 * does not count adds +0.0.  N = 0 leaves 43 zeros (the caller decides what that means).  The volumes must be finite.
 *
 * THE SUMMATION TREE is part of the definition and a function of (fz, fy, fx) alone -- not of the data, the device or
 * the launch.  The fixed volume is cut into bricks of 64 (x) x 4 (y) x 8 (z) voxels, padded with zeros.  In a brick,
 * column (x, y) adds its 8 voxels in z order starting from 0.0; the 64 columns of a row are added by halving
 * (v[i] + v[i + 32] for i < 32, then 16, .. 1); the 4 rows by halving ((r0 + r2) + (r1 + r3)): the brick's slab.  The
 * slabs, in (bz, by, bx) order, bx fastest, are reduced in passes: each group of 256 consecutive values, the last one
 * padded with zeros, is added by halving (128, 64, .. 1); passes repeat until one value is left (at least one pass).
 * No floating-point atomics.
 *
 * t2fit_register_workspace_bytes: with n_0 = ceil(fx / 64) ceil(fy / 4) ceil(fz / 8) slabs and n_{p+1} = ceil(n_p / 256)
 * while n_p > 256, the sum over the passes of up(43 * 8 * n_p), up(v) = v rounded up to 256.  Plain arithmetic, no
 * device. */
#define T2FIT_REGISTER_SUMS 43
int t2fit_register_workspace_bytes(int fz, int fy, int fx, size_t *bytes);

/* fixed_dev: float32 [fz fy fx]; fixed_mask_dev: uint8, same shape; moving_dev / moving_mask_dev likewise [mz my mx];
 * A: HOST pointer, read before the call returns; sums_dev: device float64 [43]; workspace_dev: at least
 * t2fit_register_workspace_bytes bytes, aligned to 256 (the slabs and the passes' values live there).  One launch for
 * the slabs and one per pass.  Asynchronous on `stream`; no allocation, copy or synchronisation.  Checked before HIP is
 * touched (T2FIT_E_INVALID and a message): a NULL pointer, a size < 1, more than 2^40 elements in a volume, more than
 * 2^31-1 bricks, a non-finite entry of A, volumes not aligned to 4 bytes, sums_dev not aligned to 8, a workspace that is
 * misaligned or too small. */
int t2fit_register_sums_dev(const float *fixed_dev, const uint8_t *fixed_mask_dev, int fz, int fy, int fx,
                            const float *moving_dev, const uint8_t *moving_mask_dev, int mz, int my, int mx, const double *A,
                            double *sums_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

/* A pyramid level of integer shrink factor s (1..32): out is [nz / s][ny / s][nx / s] (integer division: whole blocks
 * only, the ragged edge is dropped).  t2fit_shrink_dev: the mean of each s^3 block -- a float64 sum in (dz, dy, dx)
 * order from 0.0, divided by s^3, one rounding to float32.  t2fit_shrink_mask_dev: 1 where any voxel of the block is
 * != 0, else 0.  The level's grid has s times the spacing and its origin at the centre of the first block.
 * Asynchronous on `stream`.  Checked before HIP is touched: NULL or equal pointers, a size < 1, s outside 1..32 or
 * larger than a size, float pointers not aligned to 4 bytes. */
int t2fit_shrink_dev(const float *src_dev, int nz, int ny, int nx, int s, float *out_dev, void *stream);
int t2fit_shrink_mask_dev(const uint8_t *src_dev, int nz, int ny, int nx, int s, uint8_t *out_dev, void *stream);

/* ---- Affine registration across contrasts: the correlation ratio's sums -------------------------------------------------
 * The device half of the T1-template-onto-T2 registration behind the atlas labels (the reference runs FSL's flirt with
 * 12 degrees of freedom and the correlation-ratio cost: utils/qmri_utils.py:1011-1037).  The FIXED volume's intensities
 * are binned once per pyramid level; with N_b and S_b the count and the sum of the interpolated moving samples m over
 * the counted voxels of bin b, mu_b = S_b / N_b and phi(i) = mu_bin(i), the correlation ratio of m given the binned f is
 *   CR = 1 - (sum_b S_b^2 / N_b - (sum m)^2 / N) / (sum m^2 - (sum m)^2 / N) = 1 + C,
 * C being the correlation metric of the 43 sums with f replaced by phi; phi maximises that correlation over the functions
 * constant on each bin, so dCR/dA with the voxel set held fixed is the dC/dA of those same sums.  One evaluation is
 * t2fit_register_binned_sums_dev (N_b, S_b and the table mu) followed by t2fit_register_sums_lut_dev (the 43 sums with
 * f = mu[bin]), on one stream without a host round trip.  Metric arithmetic, the 12-parameter transform and the descent
 * are host code (fetal_t2mapping_amd/_register.py, which restates everything here in numpy; the device results equal it
 * bit for bit).  Parity with flirt is not pinned.  Additive to ABI 5: four new symbols (look them up).
 *
 * The counting rule, the interpolant m and THE SUMMATION TREE are those written above for the 43 sums.  A bin byte above
 * n_bins - 1 counts as n_bins - 1.  Checked before HIP is touched by all of them (T2FIT_E_INVALID and a message): a NULL
 * pointer (lut_dev of t2fit_register_binned_sums_dev alone may be NULL), n_bins outside 1..64, a size < 1, a non-finite
 * entry of A, lo or scale, float32 volumes not aligned to 4 bytes, float64 arrays not aligned to 8, a workspace that is
 * not aligned to 256 bytes or too small.
 *
 * t2fit_register_bin_dev: out[v] = clamp(floor(((double)src[v] - lo) * scale), 0, n_bins - 1) as uint8, every operation
 * rounding once in float64; a NaN gives 0, so scale = 0 gives all zeros.  n_vox in 1..2^39-1.  The host chooses lo = the
 * smallest and hi = the largest sample inside the fixed mask and scale = n_bins / (hi - lo), 0 when hi == lo; a sample
 * equal to hi clamps to n_bins - 1. */
int t2fit_register_bin_dev(const float *src_dev, int64_t n_vox, double lo, double scale, int n_bins, uint8_t *out_dev,
                           void *stream);

/* As t2fit_register_workspace_bytes with 2 n_bins values per slab in place of 43. */
int t2fit_register_binned_workspace_bytes(int fz, int fy, int fx, int n_bins, size_t *bytes);

/* binned_dev: device float64 [2 n_bins] = N_0 .. N_{B-1}, S_0 .. S_{B-1}.  A voxel that counts adds (1.0, m) to its own
 * bin and +0.0 to every other, all through the tree; no floating-point atomics; the order of every addition is a
 * function of (fz, fy, fx) and n_bins alone.  lut_dev: NULL, or device float64 [n_bins] that a last small kernel fills
 * with lut[b] = N_b > 0 ? S_b / N_b : 0.0.  N = 0 leaves zeros.  bins_dev: uint8 [fz fy fx]; the other arguments as for
 * t2fit_register_sums_dev; workspace_dev: at least t2fit_register_binned_workspace_bytes bytes, aligned to 256.  One
 * launch for the slabs, one per pass, one for the table.  Asynchronous on `stream`. */
int t2fit_register_binned_sums_dev(const uint8_t *bins_dev, const uint8_t *fixed_mask_dev, int fz, int fy, int fx,
                                   const float *moving_dev, const uint8_t *moving_mask_dev, int mz, int my, int mx,
                                   const double *A, int n_bins, double *binned_dev, double *lut_dev, void *workspace_dev,
                                   size_t workspace_bytes, void *stream);

/* The 43 sums of t2fit_register_sums_dev with f = lut_dev[bins_dev[i]], a float64 that is not rounded to float32 (the
 * same kernel body).  workspace_dev: at least t2fit_register_workspace_bytes bytes.  Asynchronous on `stream`. */
int t2fit_register_sums_lut_dev(const uint8_t *bins_dev, const double *lut_dev, int n_bins, const uint8_t *fixed_mask_dev,
                                int fz, int fy, int fx, const float *moving_dev, const uint8_t *moving_mask_dev, int mz,
                                int my, int mx, const double *A, double *sums_dev, void *workspace_dev,
                                size_t workspace_bytes, void *stream);

/* ---- Mattes mutual information: the joint histogram and the gradient's sums ---------------------------------------------
 * The device half of a registration by the cost that elastix's default "rigid" parameter map minimises, which is what
 * the reference's registration_elastix runs (utils/qmri_utils.py:82-91, :1039-1051): Mattes mutual information with a
 * zero-order window on the fixed image and a cubic B-spline Parzen window on the moving image.  One evaluation is
 * t2fit_register_joint_hist_dev, the metric and the table T on the host (fetal_t2mapping_amd/_register.py:
 * mattes_metric, which also restates everything here in numpy; the device results equal it bit for bit), and
 * t2fit_register_mi_gradient_dev.  Same cost and window as elastix, another sampler (every voxel that counts, not a
 * random subset per iteration) and another descent: parity with elastix is not pinned.  Additive to ABI 5:
 * three new symbols (look them up).
 *
 * The counting rule, the interpolant m, the node gradient g_a with its flat rule, u = (ix, iy, iz, 1), "every product
 * rounds once, no fused multiply-add" and THE SUMMATION TREE are those written above for the 43 sums.
 * FIXED SIDE: the uint8 bin volume of t2fit_register_bin_dev, n_f in 1..64, a byte above n_f - 1 counts as n_f - 1.
 * MOVING SIDE: n_m in 5..64 bins, two of them padding at each end.  The host chooses lo_m / hi_m = the smallest / largest
 * moving sample inside the moving mask and scale_m = (n_m - 4) / (hi_m - lo_m), 0 when they are equal.  Per counted
 * voxel, in float64, each operation rounding once and in this order:
 *   t = (m - lo_m) * scale_m + 2;  t = t >= 2 ? t : 2;  t = t <= n_m - 2 ? t : n_m - 2   (a NaN becomes 2)
 *   i0 = min(floor(t), n_m - 3);   u = t - i0;  v = 1 - u;  u2 = u u;  v2 = v v;  u3 = u2 u;  v3 = v2 v
 *   w_0 = v3 / 6    w_1 = ((3 u3 - 6 u2) + 4) / 6    w_2 = (((-3 u3 + 3 u2) + 3 u) + 1) / 6    w_3 = u3 / 6
 *   w'_0 = -(v2 0.5)    w'_1 = 1.5 u2 - 2 u    w'_2 = (-1.5 u2 + u) + 0.5    w'_3 = u2 0.5
 * w_j is the weight of bin i0 - 1 + j (the uniform cubic B-spline basis), w'_j its derivative with respect to t.  No pow,
 * nothing from libm but floor, no contraction.  m = hi_m gives i0 = n_m - 3, u = 1: bins n_m - 4 .. n_m - 1; m = lo_m
 * gives i0 = 2, u = 0: bins 1 .. 4; an m beyond the mask's range lands where the nearer of the two does.
 * JOINT HISTOGRAM: H[b_f][k], uint64 [n_f][n_m]; a counted voxel adds q_j = (uint64)floor(w_j * 2^30 + 0.5) to
 * H[b_f][i0 - 1 + j], j = 0..3.  Integer sums, exact in any order (64-bit integer atomics, LDS then global; no
 * floating-point atomics).  A fixed volume of more than 2^32 voxels is refused, so no entry can pass 2^63.
 * METRIC (host): p = H / sum H with marginals p_f, p_m; MI = sum_{p > 0} p log(p / (p_f p_m)), the cost is -MI.  sum H
 * counts in units of 2^-30 voxel, so T[b_f][k] = -(scale_m * 2^30 / sum H) log(p / p_m) where p > 0, 0 elsewhere.  With the
 * counted set held fixed p_f does not depend on the transform and sum dp = 0, hence d(-MI)/dA[a][j] = sum_v c_v g_a u_j
 * with c_v = sum_j T[b_f][i0 - 1 + j] w'_j(u), the four products added in j order from 0.0.
 * GRADIENT SUMS: float64 [12], [4 a + j] = sum (c g_a) u_j, c g_a rounded first, then u_j (u_3 = 1 is no multiplication),
 * through the tree; a voxel that does not count adds +0.0.
 *
 * Both calls are asynchronous on `stream`; no allocation, copy or synchronisation; A is a HOST pointer read before the
 * call returns.  Checked before HIP is touched (T2FIT_E_INVALID and a message): a NULL pointer, n_f outside 1..64, n_m
 * outside 5..64, a size < 1, a non-finite entry of A, lo_m or scale_m, moving_dev not aligned to 4 bytes, hist_dev /
 * table_dev / sums_dev not aligned to 8, a workspace that is not aligned to 256 bytes or too small.
 *
 * t2fit_register_joint_hist_dev zeroes hist_dev on the stream, then adds (two launches). */
#define T2FIT_REGISTER_MI_SUMS 12
int t2fit_register_joint_hist_dev(const uint8_t *bins_dev, const uint8_t *fixed_mask_dev, int fz, int fy, int fx,
                                  const float *moving_dev, const uint8_t *moving_mask_dev, int mz, int my, int mx,
                                  const double *A, int n_f, int n_m, double lo_m, double scale_m, uint64_t *hist_dev,
                                  void *stream);

/* As t2fit_register_workspace_bytes with 12 values per slab in place of 43. */
int t2fit_register_mi_workspace_bytes(int fz, int fy, int fx, size_t *bytes);

/* table_dev: device float64 [n_f][n_m]; sums_dev: device float64 [12]; workspace_dev: at least
 * t2fit_register_mi_workspace_bytes bytes, aligned to 256.  The kernel of the 43 sums with 12 accumulators and the table
 * staged in LDS; one launch for the slabs and one per pass. */
int t2fit_register_mi_gradient_dev(const uint8_t *bins_dev, const double *table_dev, int n_f, int n_m, double lo_m,
                                   double scale_m, const uint8_t *fixed_mask_dev, int fz, int fy, int fx,
                                   const float *moving_dev, const uint8_t *moving_mask_dev, int mz, int my, int mx,
                                   const double *A, double *sums_dev, void *workspace_dev, size_t workspace_bytes,
                                   void *stream);

/* ---- Non-rigid alignment: a cubic B-spline free-form deformation under Mattes mutual information -----------------------
 * The device half of a deformable step after the affine registration (the reference has none: build_jhu_ho_labels is
 * flirt with 12 degrees of freedom).  The metric arithmetic, the regulariser and the descent are host code
 * (fetal_t2mapping_amd/_ffd.py, which also restates everything here in numpy; the device results equal it bit for bit).
 * Parity with elastix, NiftyReg or ANTs is not pinned.  Additive to ABI 5: five new symbols (look them up).
 *
 * THE TRANSFORM.  For the fixed voxel x = (ix, iy, iz) the moving index coordinate is c(x) = A (x + d(x), 1) with
 *   d_k(x) = sum_z bz sum_y by sum_x bx phi_k[kz + .][ky + .][kx + .],  k = 0..2 (0 is x), in fixed-grid voxels.
 * lattice_dev is float64 [3][c][c][c], c = side in {4, 5, 7, 11, 19}.  Along an axis of n voxels the first node k and the
 * weights b_0..3 of voxel i are those of the N4 lattice above: p = (i (c - 3)) / (n - 1), k = floor(p), tau = p - k, the
 * last voxel k = c - 4, tau = 1 (n = 1: k = 0, tau = 0), b = the uniform cubic B-spline basis in tau.  The taps are added
 * z, then y, then x, each as ((w_0 v_0 + w_1 v_1) + w_2 v_2) + w_3 v_3, in float64.  With p = (ix + d_0, iy + d_1,
 * iz + d_2), c_a = ((A[4a] p_x + A[4a+1] p_y) + A[4a+2] p_z) + A[4a+3].  A lattice of zeros gives the coordinates of the
 * affine entry points bit for bit.  Every multiply and add rounds once, no fused multiply-add.
 *
 * JOINT HISTOGRAM (t2fit_ffd_joint_hist_dev): t2fit_register_joint_hist_dev with c(x) in place of A x: same counting
 * rule, same window, integer sums (64-bit integer atomics, LDS then global), equal to the statement integer for integer.
 * GRADIENT (t2fit_ffd_gradient_dev): float64 [3][c][c][c], the lattice gradient of -MI with the counted set held fixed.
 * Per counted voxel s = sum_j T[b_f][i0 - 1 + j] w'_j(u) (the c_v of t2fit_register_mi_gradient_dev), the force
 *   f_j = ((s g_0) A[j] + (s g_1) A[4 + j]) + (s g_2) A[8 + j],  s g_a rounded first,
 * +0.0 at a voxel that does not count, and G_j[cz][cy][cx] = sum_z bz sum_y by sum_x bx f_j: along x lane l of a wave adds
 * the terms l, l + 64, .. of the row in order from +0.0 and the 64 lanes halve (32, 16, .. 1); then y, then z in index
 * order from +0.0.  A node outside a voxel's four receives +0.0 from it, not a product with a zero weight: a non-finite
 * sample cannot reach a node whose support it lies outside.  No floating-point atomics; bit-identical from call to call.
 * WARP (t2fit_ffd_warp_dev): t2fit_resample_dev's sample (linear for float32, nearest for float32 / int32, default_value
 * outside, no flags, one volume) at c(x) on the output grid; with a lattice of zeros the bytes of t2fit_resample_dev.
 * JACOBIAN (t2fit_ffd_jacobian_dev): det(I + dd/dx) per voxel from the analytic derivative weights -- the derivative of
 * the basis in tau (-(om om) 0.5, 1.5 t2 - 2 tau, (-1.5 t2 + tau) + 0.5, t2 0.5), each times (c - 3) / (n - 1), 0 when
 * n = 1 -- as (a00 (a11 a22 - a12 a21) - a01 (a10 a22 - a12 a20)) + a02 (a10 a21 - a11 a20), a[k][a] = [k == a] +
 * dd_k/dx_a; *min_dev is the minimum over the voxels whose mask byte is not 0 (+Inf when there is none), *n_folded_dev the
 * count of det <= 0 among them.  Minimum and count do not depend on the order.  A lattice of zeros gives exactly 1.0 and 0.
 *
 * All calls are asynchronous on `stream`; no allocation, copy or synchronisation; A is a HOST pointer read before the
 * call returns.  workspace_dev: at least t2fit_ffd_workspace_bytes(fixed sizes, side) bytes, aligned to 256 (the axis
 * tables, the row and plane sums of the gradient, the row minima and counts); calls that may overlap need one each.
 * Checked before HIP is touched (T2FIT_E_INVALID and a message): a NULL pointer, a side that is not one of the five,
 * n_f outside 1..64, n_m outside 5..64, a size < 1, a non-finite entry of A, lo_m or scale_m, an unknown src_type / interp,
 * an int32 source with linear interpolation, a default_value that does not fit int32, moving_dev / src_dev / out_dev not
 * aligned to 4 bytes, lattice_dev / hist_dev / table_dev / grad_dev / min_dev / n_folded_dev not aligned to 8, out_dev =
 * src_dev, grad_dev = lattice_dev, a workspace that is not aligned to 256 bytes or too small. */
int t2fit_ffd_workspace_bytes(int fz, int fy, int fx, int side, size_t *bytes);

int t2fit_ffd_joint_hist_dev(const uint8_t *bins_dev, const uint8_t *fixed_mask_dev, int fz, int fy, int fx,
                             const float *moving_dev, const uint8_t *moving_mask_dev, int mz, int my, int mx,
                             const double *A, const double *lattice_dev, int side, int n_f, int n_m, double lo_m,
                             double scale_m, uint64_t *hist_dev, void *workspace_dev, size_t workspace_bytes, void *stream);

int t2fit_ffd_gradient_dev(const uint8_t *bins_dev, const double *table_dev, int n_f, int n_m, double lo_m, double scale_m,
                           const uint8_t *fixed_mask_dev, int fz, int fy, int fx, const float *moving_dev,
                           const uint8_t *moving_mask_dev, int mz, int my, int mx, const double *A,
                           const double *lattice_dev, int side, double *grad_dev, void *workspace_dev,
                           size_t workspace_bytes, void *stream);

/* src_type: T2FIT_RESAMPLE_F32 / _I32; interp: T2FIT_INTERP_LINEAR / _NEAREST; (nz, ny, nx) the source, (oz, oy, ox) the
 * output (fixed) grid the lattice spans. */
int t2fit_ffd_warp_dev(const void *src_dev, int src_type, int nz, int ny, int nx, const double *A,
                       const double *lattice_dev, int side, void *out_dev, int oz, int oy, int ox, int interp,
                       double default_value, void *workspace_dev, size_t workspace_bytes, void *stream);

int t2fit_ffd_jacobian_dev(const double *lattice_dev, int side, const uint8_t *mask_dev, int fz, int fy, int fx,
                           double *min_dev, int64_t *n_folded_dev, void *workspace_dev, size_t workspace_bytes,
                           void *stream);

/* ---- Slice-to-volume registration: the 43 sums of every slice of every stack, batched ------------------------------------
 * The device half of the step that finds the per-slice poses t2fit_sr_slice_*_dev consume: one launch evaluates the
 * correlation metric's 43 sums of K slices, each slice of each stack under an affine of its own, against one volume.  The
 * metric arithmetic, the transform model and the descent that advances all slices in lockstep are host code
 * (fetal_t2mapping_amd/_svr.py, which also restates everything here in numpy; the device results equal it bit for bit;
 * DESIGN.md 8l).  Additive to ABI 5: four new symbols (look them up).
 *
 * PER SLICE.  The fixed image is plane k of stack s, float32 [ly][lx], with the stack's mask plane (a NULL mask: all ones);
 * the moving image is the volume [mz][my][mx] with its mask (NULL: all ones).  A_k (12 doubles, the order of evaluation of
 * t2fit_resample_dev) maps the slice index (ix, iy, k) to a continuous index of the volume.  The counting rule, f, m, g_a,
 * the flat-gradient rule, the 43 terms and their rounding order are those of t2fit_register_sums_dev with
 * u = (ix, iy, k, 1): u_z is the slice's index in its stack.  A voxel that does not count adds +0.0; slot 42 stays +0.0.
 *
 * THE SLICE TREE is a function of (ly, lx) alone and differs from the volume's on purpose (a slice has no z to walk).
 * The slice is cut into bricks of 64 (x) x 32 (y) voxels, padded with zeros.  In a brick, column x of row group w (0..3)
 * adds its rows y = 32 by + 8 w + r, r = 0..7, in order starting from 0.0; the 64 columns of a row group are added by
 * halving; the 4 row groups as (w0 + w2) + (w1 + w3): the brick's slab.  The slabs, in (by, bx) order, bx fastest, are
 * reduced in the passes of 256 written above for t2fit_register_sums_dev.  In a batch every slice is padded with slabs of
 * +0.0 up to the largest slab count of any stack; adding +0.0 changes no bit of a sum.
 *
 * THE TABLE: a record of T2FIT_SVR_RECORD_BYTES = 128 bytes per slice, record r at byte 128 r: A[12] float64, then int32
 * stack, slice, active, and 5 pad words of 0.  Records may come in any order and a (stack, slice) pair more than once.
 * sums_dev: device float64 [n_slices][43], row r for record r.  A record with active == 0, or whose stack index is outside
 * 0 .. n_stacks - 1 or whose slice index is outside its stack, gives a row of +0.0: the table is data, not a trusted
 * argument, and whatever it holds the kernel ends and stays inside its buffers.  A non-finite A counts no voxel (the
 * inside test is false for NaN).  t2fit_svr_table_host packs the table on the host (no device) and refuses, before it
 * writes a byte: a NULL pointer, n_slices < 1, n_stacks outside 1 .. T2FIT_SR_MAX_STACKS, a size < 1, a non-finite A, a
 * stack or slice index out of range, a buffer smaller than t2fit_svr_table_bytes says.  lo_size: int32 [n_stacks][3] =
 * (lz, ly, lx).
 *
 * t2fit_svr_workspace_bytes: with n_0 = the largest ceil(lx / 64) ceil(ly / 32) of any stack and n_{p+1} = ceil(n_p / 256)
 * while n_p > 256, the sum over the passes of up(43 * 8 * n_slices * n_p), up(v) = v rounded up to 256.
 *
 * t2fit_svr_sums_dev: fixed_dev / fixed_mask_dev are HOST arrays of n_stacks device pointers (fixed_mask_dev or an entry
 * of it may be NULL: all ones); one launch for the slabs, one per pass (split where 43 n_slices exceeds a grid's y
 * extent).  Asynchronous on `stream`; no allocation, copy or synchronisation.  Checked before HIP is touched
 * (T2FIT_E_INVALID and a message): a NULL pointer, n_stacks outside 1 .. T2FIT_SR_MAX_STACKS, n_slices < 1, a size < 1,
 * more than 2^40 elements in a stack or the volume, more than 2^31-1 workgroups, float pointers not aligned to 4 bytes,
 * sums_dev or table_dev not aligned to 8, a workspace that is not aligned to 256 bytes or too small. */
#define T2FIT_SVR_RECORD_BYTES 128
int t2fit_svr_table_bytes(int n_slices, size_t *bytes);
int t2fit_svr_table_host(int n_slices, const double *A /* [n][12] */, const int32_t *stack, const int32_t *slice,
                         const uint8_t *active, int n_stacks, const int32_t *lo_size, void *table_host, size_t bytes);
int t2fit_svr_workspace_bytes(int n_stacks, const int32_t *lo_size, int n_slices, size_t *bytes);
int t2fit_svr_sums_dev(int n_stacks, const float *const *fixed_dev, const uint8_t *const *fixed_mask_dev,
                       const int32_t *lo_size, const float *moving_dev, const uint8_t *moving_mask_dev, int mz, int my,
                       int mx, const void *table_dev, int n_slices, double *sums_dev, void *workspace_dev,
                       size_t workspace_bytes, void *stream);

/* ---- N4 bias-field correction: log image, sharpening histogram, B-spline fit, field -------------------------------------
 * The device half of the reference's run_biasfield_correction / run_biasfield_correction2 (utils/qmri_utils.py:254-357),
 * which call sitk.N4BiasFieldCorrectionImageFilter.  The definition is written from the N4 paper (Tustison 2010), the
 * multilevel B-spline paper (Lee, Wolberg and Shin 1997) and ITK's documentation; PARITY WITH ITK IS UNPINNED (DESIGN.md
 * 8h).  The sharpening table, the lattice refinement, the convergence figure and the loop are host code
 * (fetal_t2mapping_amd/_bias.py, which also restates everything here in numpy; the device results equal it bit for bit
 * wherever no transcendental is involved).  Additive to ABI 5: eight new symbols (look them up).
 *
 * Every per-voxel volume is float32 [nz ny nx] in memory; all arithmetic is float64, every multiply and add rounding once
 * (no fused multiply-add), one rounding at a float32 store.  Inputs must be finite.
 *
 * 1. LOG IMAGE.  M = mask != 0 and in > 0 (mask NULL: in > 0); u0 = (float)log((double)in) in M, +0.0 elsewhere.  The
 *    loop starts from u = u0, field = 0 and a lattice L of zeros of side 4.
 * 2. SHARPENING.  lo, hi = min, max of u over M; slope = (hi - lo) / (B - 1), B bins (200).  The bin coordinate of a
 *    voxel: c = clamp(((double)u - lo) / slope, 0, B - 1), i = min(floor(c), B - 2), t = c - i.  The histogram is fixed
 *    point: w = floor(t 2^24 + 0.5), H[i] += 2^24 - w, H[i + 1] += w in uint64 -- integer adds, exact in any order (a
 *    stated departure from ITK's float histogram: 6e-8 of a voxel).  From H the host makes the table E[B] (the histogram
 *    deconvolved by a Gaussian of full width fwhm with a Wiener filter, then the expected true value per bin).  The
 *    sharpened value of a voxel is E[i] (1 - t) + E[i + 1] t and its residual r = (double)u - that, in M.
 * 3. FIT, one level of multilevel B-spline approximation on a lattice of side c (4, 5, 7, 11, 19 by level).  Along an
 *    axis of n voxels: s = c - 3, p = (i s) / (n - 1), k = floor(p), tau = p - k; for i = n - 1: k = s - 1, tau = 1; for
 *    n = 1: k = 0, tau = 0.  The uniform cubic B-spline weights at nodes k .. k + 3, every other weight 0:
 *      b0 = ((1 - tau)^2 (1 - tau)) / 6        b1 = ((3 tau^3 - 6 tau^2) + 4) / 6
 *      b2 = (((-3 tau^3 + 3 tau^2) + 3 tau) + 1) / 6        b3 = tau^3 / 6        (tau^2 = tau tau, tau^3 = tau^2 tau)
 *    q = b b, S = ((q0 + q1) + q2) + q3, a = (q b) / S.  Over the voxels of M,
 *      delta[cz][cy][cx] = sum az ay ax r        omega[cz][cy][cx] = sum qz qy qx
 *    contracted x first, then y, then z; the lattice increment is delta / omega, 0 where omega = 0: L += delta / omega.
 *    THE ORDER OF SUMMATION is part of the definition.  The x contraction of a row (z, y) and node cx takes the terms
 *    ax r (q for omega) in x order, zero-padded to a multiple of 64: lane l adds terms l, l + 64, .. in order from +0.0,
 *    then the 64 lanes halve (v[i] + v[i + 32] for i < 32, then 16, .. 1).  The y and the z contraction add weight times
 *    partial sum in index order from +0.0.  omega depends on M and the level only.
 * 4. FIELD, at every voxel: T1[z][cy][cx] = ((bz0 L[kz] + bz1 L[kz + 1]) + bz2 L[kz + 2]) + bz3 L[kz + 3], T2[z][y][cx]
 *    likewise from T1 along y, field = (float)(likewise from T2 along x).
 * 5. CONVERGENCE.  d = expm1((double)field_new - (double)field_old) over M; sum d and sum d d per row by the lanes and
 *    the halving of step 3, the rows in (z, y) order by passes of 256-to-1 halving groups (the last group padded with
 *    zeros, at least one pass: the tree of t2fit_register_sums_dev).  Then u = (float)((double)u0 - (double)field_new)
 *    in M, +0.0 elsewhere.  The host forms conv = sqrt((sum dd - (sum d)^2 / N) / (N - 1)) / (1 + sum d / N).
 * 6. NEXT LEVEL: the host refines L by cubic subdivision (side c -> 2 c - 3; the field is unchanged).
 * 7. OUTPUT: out = (float)(((double)in / exp((double)field)) scale) at every voxel.
 * No floating-point atomics anywhere.  log, expm1 and exp are the device library's: results that pass through one may
 * differ from another library's in the last bit.
 *
 * All pointers but `bytes` are device pointers.  Every entry point is asynchronous on `stream`, allocates and copies
 * nothing, and checks every argument before HIP is touched (T2FIT_E_INVALID and a message): a NULL pointer (mask_dev of
 * t2fit_n4_log_dev and table_dev of t2fit_n4_fit_dev alone may be NULL), a size < 1, more than 2^31-1 rows (nz ny) or
 * 2^40 elements, n_vox outside 1..2^39-1, a lattice side that is not 4, 5, 7, 11 or 19, bins outside 2..1024, lo, slope
 * or scale not finite, slope <= 0, float32 arrays not aligned to 4 bytes, float64 and uint64 arrays not aligned to 8,
 * arrays that must differ being the same, a workspace that is NULL, not aligned to 256 bytes or too small.
 *
 * t2fit_n4_workspace_bytes: one workspace serves every entry point below for a volume and a side (the axis tables, the
 * row sums of the x contraction [nz ny][c], the y contraction [nz][c][c], the rows' minima and maxima and the passes of
 * the tree, each part rounded up to 256 bytes; never less than 8192).  Plain arithmetic, no device.  The entry points keep
 * nothing in it between calls: it may hold anything, NaN included, when a call starts. */
int t2fit_n4_workspace_bytes(int nz, int ny, int nx, int side, size_t *bytes);

/* Step 1.  u0_dev: float32 [n_vox], m_dev: uint8 [n_vox] (0 / 1); u0_dev must not be in_dev. */
int t2fit_n4_log_dev(const float *in_dev, const uint8_t *mask_dev, int64_t n_vox, float *u0_dev, uint8_t *m_dev, void *stream);

/* range_dev: float32 [2] = min, max of u over M (+inf, -inf when M is empty).  workspace_dev: at least 8192 bytes. */
int t2fit_n4_minmax_dev(const float *u_dev, const uint8_t *m_dev, int64_t n_vox, float *range_dev, void *workspace_dev,
                        size_t workspace_bytes, void *stream);

/* Step 2's histogram: hist_dev uint64 [bins], zeroed and filled by the call (a per-workgroup histogram in LDS, then
 * integer atomics).  The sum of hist_dev is 2^24 times the voxels of M. */
int t2fit_n4_histogram_dev(const float *u_dev, const uint8_t *m_dev, int64_t n_vox, double lo, double slope, int bins,
                           uint64_t *hist_dev, void *stream);

/* Step 3's omega: omega_dev float64 [side^3]. */
int t2fit_n4_weights_dev(const uint8_t *m_dev, int nz, int ny, int nx, int side, double *omega_dev, void *workspace_dev,
                         size_t workspace_bytes, void *stream);

/* Step 3: delta_dev float64 [side^3] is written, lattice_dev float64 [side^3] is updated in place with omega_dev (of
 * t2fit_n4_weights_dev for the same M and side).  table_dev: float64 [bins], the table E; NULL: r = u (lo, slope and
 * bins are then ignored), which fits u itself. */
int t2fit_n4_fit_dev(const float *u_dev, const uint8_t *m_dev, int nz, int ny, int nx, const double *table_dev, double lo,
                     double slope, int bins, int side, const double *omega_dev, double *lattice_dev, double *delta_dev,
                     void *workspace_dev, size_t workspace_bytes, void *stream);

/* Steps 4 and 5: field_dev holds the old field and receives the new one; u_dev receives the new u; sums_dev float64 [2]
 * = sum d, sum d d; range_dev float32 [2] = min, max of the new u over M, so the next iteration needs no range pass. */
int t2fit_n4_field_dev(const double *lattice_dev, int side, const float *u0_dev, const uint8_t *m_dev, int nz, int ny, int nx,
                       float *field_dev, float *u_dev, double *sums_dev, float *range_dev, void *workspace_dev,
                       size_t workspace_bytes, void *stream);

/* Step 7; out_dev may be in_dev, not field_dev. */
int t2fit_n4_apply_dev(const float *in_dev, const float *field_dev, int64_t n_vox, double scale, float *out_dev, void *stream);

/* ---- Dictionary-matching fit (additive to ABI 5) ---------------------------------------------------------------------
 * Any signal model as a table: A atoms (decay curves) of n_te samples each.  Every voxel's decay is matched against every
 * atom; the best atom gives the parameters (the caller's table, row `index`), the projection onto it the scale.  With
 * D the atoms as given (float32), everything below float64 with one rounding per operation in the order written, nothing
 * fused, sums over the echoes e ascending from 0.0:
 *   packing   n2_j = sum_e D_je D_je, n_j = sqrt(n2_j), Dh_je = float32(D_je / n_j),
 *             dmax = float32(max_j sqrt(sum_e Dh_je Dh_je))
 *   score     s_j = sum_e Dh_je y_e;  index = argmax_j s_j, the lowest j on a tie
 *   scale     q = (sum_e y_e D_je) / n2_j of the matched atom, k = q if q > 0 else 0;  scale = float32(k)
 *   rmse      float32(sqrt((sum_e (y_e - k D_je)^2) / n_te))
 * A voxel with mask == 0 or a non-finite sample is not fitted: index -1, scale 0, rmse 0.  An all-zero voxel ties on every
 * atom: index 0, scale 0, rmse 0.  fetal_t2mapping_amd/_dict.py states all of it in numpy; the device output is
 * bit-identical to it.  (The device finds candidates with the float32 matrix instruction and re-scores, in float64 as
 * above, every atom whose float32 score is within a proven error bound of the running best: DESIGN.md section 8r.)
 *
 * The packed dictionary is one block of t2fit_dict_pack_bytes bytes, little endian, that t2fit_dict_pack_host writes on
 * the host and the caller copies to the device (16-byte aligned) once per dictionary:
 *   byte  0  uint32 magic 0x54443254   int32 n_atoms   int32 n_te   int32 k_pad (n_te rounded up to even)
 *   byte 16  int32 n_tiles (ceil(n_atoms / 32))   float32 dmax   uint32 0, 0
 *   byte 32  uint64 off_tiles (= 64)   uint64 off_atoms   uint64 off_norm2   uint64 bytes (the whole block)
 *   off_tiles  float32 [n_tiles][k_pad][32]: Dh of atom 32 t + r at [t][e][r]; 0.0 for e >= n_te and for 32 t + r >= n_atoms
 *   off_atoms  float32 [n_atoms][n_te]: D as given; the section is padded with zero bytes to a multiple of 16
 *   off_norm2  float64 [n_atoms]: n2_j; padded likewise */
#define T2FIT_DICT_MAX_ATOMS 65536 /* n_atoms outside 1 .. this is refused; n_te outside 2 .. T2FIT_MAX_TE likewise */

/* Plain arithmetic, no device. */
int t2fit_dict_pack_bytes(int n_atoms, int n_te, size_t *bytes);

/* No device.  atoms: float32 [n_atoms][n_te] on the host.  Refuses (T2FIT_E_INVALID, with a message) the sizes above, a NULL
 * pointer, `bytes` below t2fit_dict_pack_bytes, an atom with a non-finite sample and an atom whose norm is 0. */
int t2fit_dict_pack_host(int n_atoms, int n_te, const float *atoms, void *packed_host, size_t bytes);

/* y_dev: float32, TE-major (n_te, n_vox).  mask_dev: uint8 [n_vox], 0 / not 0, or NULL (every voxel).  index_dev int32,
 * scale_dev and rmse_dev float32, [n_vox] each, all written for every voxel.  One kernel on `stream`, no allocation.
 * Refused before HIP is touched: a NULL y_dev, packed_dev or output, n_te outside 2 .. T2FIT_MAX_TE, n_vox < 0, y_dev or an
 * output not aligned to 4 bytes, packed_dev not aligned to 16.  The 64-byte header is then read back from packed_dev (one
 * copy and one wait on `stream`: the only synchronisation) and refused, before any launch, when its magic, n_te, k_pad,
 * n_atoms, n_tiles or offsets are not what t2fit_dict_pack_host writes for this n_te.  n_vox == 0 is a no-op. */
int t2fit_dict_match_dev(const float *y_dev, int n_te, int64_t n_vox, const uint8_t *mask_dev, const void *packed_dev,
                         int32_t *index_dev, float *scale_dev, float *rmse_dev, void *stream);

/* ---- Gibbs-ringing removal by local sub-voxel shifts (additive to ABI 5) ----------------------------------------------
 * Kellner et al. 2016 on float32 slices (S, ny, nx), every slice on its own, the in-plane axes last.  Refused:
 * nx or ny outside T2FIT_UNRING_MIN_N .. T2FIT_UNRING_MAX_N, K outside 1 .. T2FIT_UNRING_MAX_SHIFTS, a window outside
 * 1 <= min_w <= max_w <= T2FIT_UNRING_MAX_WINDOW, min(nx, ny) < 2 (max_w + 1) + 1.  fetal_t2mapping_amd/_unring.py states
 * everything below in numpy; the device output is bit-identical to it and equal from call to call.
 *
 * Tables: built on the host in float64 and rounded once to float32 (t2fit_unring_tables_host; _unring.Tables.pack writes
 * the same block).  The device calls read them, so a caller may pass either.  The block, little endian, 16-byte aligned
 * on the device:
 *   byte   0  uint32 magic 0x52553254   int32 nx   int32 ny   int32 K   16 bytes 0
 *   byte  32  uint64 offsets of cx, sx, cy, sy, g, hx, hy, ab   uint64 bytes (the whole block)   24 bytes 0
 *   cx, sx    float32 [nx][nx]: C[k][m] = cos(2 pi ((k m) mod nx) / nx), S likewise with sin;  cy, sy: the same for ny
 *   g         float32 [ny][nx]: G = cy / (cx + cy) with cx = 1 + cos(2 pi kx / nx), cy = 1 + cos(2 pi ky / ny), 0.5 where
 *             cx + cy = 0; stored as float32(G / (nx ny))
 *   hx, hy    float32 [2K+1][n]: the taps of the shifts s_0 = 0, s_j = j / (2K+1), s_{K+j} = -j / (2K+1) (j = 1 .. K):
 *             h_j[d] = (1/n) [1 + 2 sum_{k=1}^{ceil(n/2)-1} cos(2 pi k (d + s_j) / n) + (n even) cos(pi d) cos(pi s_j)];
 *             row 0 is (1, 0, 0, ..) and is never read
 *   ab        float32 [2][2K+1]: a_j = float32(1 - |s_j|), then b_j = float32(|s_j|)
 *   every table is padded with zero bytes to a multiple of 16.
 *
 * Arithmetic: every product of a table and data is a float32 fma chain over the contracted index, ascending, from 0.0f
 * (what v_mfma_f32_32x32x2_f32 computes; an odd length is padded with exact zeros).  Everything else is float32 with one
 * rounding per operation, nothing fused.
 *
 * Step 1, split (t2fit_unring_split_dev).  Planes are indexed [y or ky][x or kx]; stacked operands hold the cosine or
 * real part first, the sine or imaginary part second, and the contracted index of a stacked operand runs through the
 * first part, then the second:
 *   [P; Q] = [Cx; Sx] . X^T (over x);   [A; B] = [[Cy, -Sy], [Sy, Cy]] . [P; Q] (over (part, y));   A, B <- fl(A G), fl(B G);
 *   [Vr; Vi] = [[Cy, Sy], [Sy, -Cy]] . [A; B] (over (part, ky));   I1 = [Cx, -Sx] . [Vr; Vi]^T (over (part, kx));   I2 = fl(X - I1).
 * I1 keeps the ringing along x, I2 the ringing along y.
 * Step 2, rows (t2fit_unring_rows_dev, along x or along y).  The shifts are visited in the order j = 0, 1, .., 2K.  Y_0 is
 * the row itself; Y_j[l] = sum_m h_j[(l - m) mod n] x[m] (the chain, over m).  d[l] = |Y_j[l] - Y_j[l-1]| (indices circular),
 * tvl[l] = sum_{t=min_w..max_w} d[l-t], tvr[l] = sum_t d[l+t+1], both ascending in t from 0.0f, tv = min(tvl, tvr).  A shift
 * replaces the running best only when its tv is strictly smaller.  The output of the winner j: Y_0[l] for j = 0,
 * fl(fl(Y_j[l] a_j) + fl(Y_j[l-1] b_j)) for s_j > 0, fl(fl(Y_j[l] a_j) + fl(Y_j[l+1] b_j)) for s_j < 0.
 * Step 3: out = rows along x of I1 + rows along y of I2, one float32 addition.
 * t2fit_unring_dev copies a slice with a non-finite sample through unchanged and counts it in *skipped; a slice whose
 * samples are all equal is copied through too (it comes back bit for bit) and is not counted.  The split and the rows on
 * their own do not look for non-finite samples: what they give on a row that holds one is not defined bit for bit. */
#define T2FIT_UNRING_MIN_N 8
#define T2FIT_UNRING_MAX_N 512
#define T2FIT_UNRING_MAX_SHIFTS 32
#define T2FIT_UNRING_MAX_WINDOW 8

typedef struct t2fit_unring_params {
  int32_t K;     /* shifts per side: 2K+1 candidates.  Default 20 */
  int32_t min_w; /* the window of the total variation, in samples.  Default 1 */
  int32_t max_w; /* default 3 */
  int32_t flags; /* 0 */
} t2fit_unring_params;

int t2fit_unring_params_default(t2fit_unring_params *params);

/* Plain arithmetic, no device. */
int t2fit_unring_tables_bytes(int ny, int nx, int K, size_t *bytes);

/* No device.  Writes the block described above; refuses the sizes above, a NULL pointer, `bytes` below
 * t2fit_unring_tables_bytes. */
int t2fit_unring_tables_host(int ny, int nx, int K, void *tables_host, size_t bytes);

/* One workspace serves t2fit_unring_split_dev and t2fit_unring_dev for up to n_slices slices: six float32 images of at
 * most 64 slices (the calls work through the slices 64 at a time) and two bytes per slice.  It does not depend on K: the
 * shifted copies never reach global memory.  Plain arithmetic, no device.  The calls keep nothing in it between calls. */
int t2fit_unring_workspace_bytes(const t2fit_unring_params *params, int n_slices, int ny, int nx, size_t *bytes);

/* X -> I1, I2, float32 [n_slices][ny][nx] each; the three must differ.  Four launches per 64 slices on `stream`.  Refused
 * before HIP is touched: a NULL pointer, the sizes above, n_slices < 0, an image not aligned to 4 bytes, tables_dev not
 * aligned to 16, a workspace that is NULL, not aligned to 256 bytes or too small.  The 128-byte header is then read back
 * from tables_dev (one copy and one wait on `stream`) and refused, before any launch, when it is not what
 * t2fit_unring_tables_host writes for this nx and ny.  n_slices == 0 is a no-op. */
int t2fit_unring_split_dev(const void *tables_dev, const float *in_dev, int n_slices, int ny, int nx, float *i1_dev, float *i2_dev,
                           void *workspace_dev, size_t workspace_bytes, void *stream);

/* Step 2 on every row (axis 0: along x) or every column (axis 1: along y, by addressing) of in_dev.  out_dev float32,
 * shift_dev int8 (the winning j) and tv_dev float32 (the winning tv), [n_slices][ny][nx] each; shift_dev and tv_dev may be
 * NULL.  out_dev must not be in_dev.  One launch, no workspace.  Refusals as above, except that the size limits and the
 * window's hold for the axis the rows run along only (across it any size from 1 to T2FIT_UNRING_MAX_N goes, and the tables
 * need to match along the axis only); params.K must be the tables' K. */
int t2fit_unring_rows_dev(const t2fit_unring_params *params, const void *tables_dev, const float *in_dev, int n_slices, int ny, int nx,
                          int axis, float *out_dev, int8_t *shift_dev, float *tv_dev, void *stream);

/* The whole stage.  shift_dev int8 and tv_dev float32, [2][n_slices][ny][nx] (axis x first), or NULL; they hold what the
 * rows gave, also for a slice that is copied through.  skipped (host) receives the number of slices with a non-finite
 * sample, or is NULL (the call then does not wait for the stream a second time).  out_dev must not be in_dev. */
int t2fit_unring_dev(const t2fit_unring_params *params, const void *tables_dev, const float *in_dev, int n_slices, int ny, int nx,
                     float *out_dev, int8_t *shift_dev, float *tv_dev, int64_t *skipped, void *workspace_dev, size_t workspace_bytes,
                     void *stream);

/* ---- Multi-component T2 spectra: regularised non-negative least squares (additive to ABI 5) ---------------------------
 * A decay y (n_te samples) is decomposed over a basis A[n_te][n_basis] (any table; exp(-TE_i / T2_j) for a T2 spectrum):
 *   min |A x - y|^2 + mu^2 |x|^2,  x >= 0     (Whittall & MacKay 1989; mu absolute, in the units of A)
 * by Lawson-Hanson's active-set method on the normal equations (Bro & de Jong 1997).  fetal_t2mapping_amd/_nnls.py states
 * all of it in numpy; the device output is bit-identical to it.  Everything is float64 with one rounding per operation in
 * the order written, nothing fused; division and square root are IEEE.  With G = A^T A + mu^2 I (every element a sum over
 * i ascending from 0.0, then mu * mu added to the diagonal; formed once by t2fit_nnls_pack_host) and the passive set P an
 * ORDERED LIST, in order of insertion, per voxel:
 *   1  h_j = sum_i A[i][j] y_i, i ascending from 0.0;  tol = tol_rel max_j |h_j|;  x = 0, P empty, nit = 0
 *   2  w_j = h_j - sum_{k in P, list order} G[j][P_k] x_k, one product subtracted at a time.  The candidate is the j not in P
 *      and not banned with the largest w_j > tol, the lowest j on a tie.  None: done.  nit == max_iter: status MAXITER,
 *      done.  Else nit += 1.
 *   3  Append j to P (position r).  L[r][c] = (G[P_r][P_c] - sum_{k<c, ascending} L[r][k] L[c][k]) / L[c][c];
 *      d = G[P_r][P_r] - sum_{k<r} L[r][k]^2.  Unless d > piv_rel G[P_r][P_r]: drop j from P, ban it until the next
 *      successful insertion, go to 2.  Else L[r][r] = sqrt(d) and the ban list is cleared.
 *   4  L z = h_P, k ascending: z_r = (h_{P_r} - sum_{k<r} L[r][k] z_k) / L[r][r];  L^T s = z, k DESCENDING:
 *      s_r = (z_r - sum_{k = p-1 .. r+1} L[k][r] s_k) / L[r][r].
 *   5  Every s_r > 0: x_P = s, go to 2.
 *   6  Else alpha = min over {r: not s_r > 0} of x_r / (x_r - s_r) (a 0 / 0 counts as 0), q the first list position that
 *      attains it.  x_q = 0 exactly, every other x_r + alpha (s_r - x_r); every entry not above 0 leaves P, the order of the
 *      rest is kept.  P empty: go to 2.  Else the factor of the new list (rows before the first removed position are
 *      unchanged); a pivot failure here: status BREAKDOWN, done with the current x.  Go to 4.
 * Outputs, float32 unless noted: x (n_basis planes, optional);  func_m = sum_j W[m][j] x_j and amp = sum_j x_j, all j
 * ascending from 0.0;  rmse = sqrt((sum_i r_i^2) / n_te) with r_i = y_i - sum_{k in P, list order} A[i][P_k] x_k, one product
 * at a time, i ascending;  nit and status, int32.  A voxel with mask == 0: all 0, status MASKED.  A voxel with a non-finite
 * sample: all 0, status NONFINITE.
 *
 * The packed basis is one block of t2fit_nnls_pack_bytes bytes, little endian, that t2fit_nnls_pack_host writes on the
 * host and the caller copies to the device (16-byte aligned) once per basis:
 *   byte  0  uint32 magic 0x4C4E3254   int32 n_te   int32 n_basis   int32 n_func
 *   byte 16  float64 mu   uint64 off_a (= 64)   uint64 off_g   uint64 off_w   uint64 bytes (the whole block)   uint64 0
 *   off_a  float64 [n_te][n_basis]: A as given      off_g  float64 [n_basis][n_basis]: G      off_w  float64 [n_func][n_basis]: W
 *   every section is padded with zero bytes to a multiple of 16 */
#define T2FIT_NNLS_MAX_BASIS 64 /* n_basis outside 2 .. this is refused; n_te outside 2 .. T2FIT_MAX_TE likewise */
#define T2FIT_NNLS_MAX_FUNC 8   /* n_func outside 0 .. this is refused */
/* Informational, not part of the interface: how this build of the kernel is tuned.  No argument and no result depends on
 * them; a later build may change them (and what t2fit_nnls_workgroup reports) without an ABI change.  The tests and the
 * benchmark tool read them to name the voxel counts at which the persistent grid changes behaviour. */
#define T2FIT_NNLS_CHUNK 64     /* consecutive voxels a wave of the persistent grid takes at a time */
#define T2FIT_NNLS_MAX_WAVES 8  /* waves of a workgroup at most; each has one voxel in flight */
#define T2FIT_NNLS_MASKED (-1)
#define T2FIT_NNLS_OK 0
#define T2FIT_NNLS_MAXITER 1
#define T2FIT_NNLS_BREAKDOWN 2
#define T2FIT_NNLS_NONFINITE 3

typedef struct t2fit_nnls_params {
    double tol_rel;     /* 1e-10 */
    double piv_rel;     /* 1e-12 */
    int32_t max_iter;   /* 0: 3 n_basis */
    int32_t max_blocks; /* 0: as many workgroups as the device holds; > 0 caps the persistent grid (never changes a result) */
} t2fit_nnls_params;

int t2fit_nnls_params_default(t2fit_nnls_params *params);

/* Plain arithmetic, no device, informational like the two constants above: the launch shape t2fit_nnls_dev uses for this
 * n_basis: the waves of a workgroup, its LDS bytes, and the workgroups a CU holds (by 160 KiB of LDS and 32 wave slots).
 * Refused: a NULL pointer, n_basis outside 2 .. T2FIT_NNLS_MAX_BASIS. */
int t2fit_nnls_workgroup(int n_basis, int *waves, size_t *lds_bytes, int *workgroups_per_cu);

/* Plain arithmetic, no device. */
int t2fit_nnls_pack_bytes(int n_te, int n_basis, int n_func, size_t *bytes);

/* No device.  basis: float64 [n_te][n_basis], functionals: float64 [n_func][n_basis] (NULL goes with n_func == 0), on the
 * host.  Refuses (T2FIT_E_INVALID, with a message) the sizes above, a NULL pointer, `bytes` below t2fit_nnls_pack_bytes, a
 * mu that is negative or not finite, and a non-finite entry of the basis or of a functional. */
int t2fit_nnls_pack_host(int n_te, int n_basis, int n_func, const double *basis, double mu, const double *functionals,
                         void *packed_host, size_t bytes);

/* y_dev: float32, TE-major (n_te, n_vox).  mask_dev: uint8 [n_vox], 0 / not 0, or NULL (every voxel).  x_dev: float32
 * (n_basis, n_vox) or NULL (not written); func_dev: float32 (n_func, n_vox), may be NULL when the basis has no functional;
 * amp_dev, rmse_dev float32, nit_dev, status_dev int32, [n_vox] each.  All are written for every voxel.  One kernel on
 * `stream` (a persistent grid that takes voxels from a counter, allocated and freed in stream order).  Refused before HIP is
 * touched: a NULL params, y_dev, packed_dev or mandatory output, n_te outside 2 .. T2FIT_MAX_TE, n_vox < 0, a tol_rel or
 * piv_rel that is negative or not finite, a negative max_iter or max_blocks, y_dev or an output not aligned to 4 bytes,
 * packed_dev not aligned to 16.  The 64-byte header is then read back from packed_dev (one copy and one wait on `stream`:
 * the only synchronisation) and refused, before any launch, when its magic, n_te, sizes, mu or offsets are not what
 * t2fit_nnls_pack_host writes for this n_te.  n_vox == 0 is a no-op. */
int t2fit_nnls_dev(const t2fit_nnls_params *params, const float *y_dev, int n_te, int64_t n_vox, const uint8_t *mask_dev,
                   const void *packed_dev, float *x_dev, float *func_dev, float *amp_dev, float *rmse_dev, int32_t *nit_dev,
                   int32_t *status_dev, void *stream);

/* ---- The chi^2 rule: the regularisation chosen per voxel (additive to ABI 5) ------------------------------------------------
 * The weight that suits a voxel depends on its signal-to-noise ratio, so mu is raised per voxel until the misfit is a set
 * factor above the unregularised misfit (Whittall & MacKay 1989; Prasloski 2012; DECAES's Chi2Factor).  Below, S(mu) is
 * the fit above with G = A^T A + mu^2 I (mu * mu added to the diagonal elements of A^T A: the G that t2fit_nnls_pack_host
 * forms for that mu, bit for bit) and ss its misfit sum_i r_i^2 as formed for the RMSE.  Everything is float64, one rounding
 * per operation in the order written; fetal_t2mapping_amd/_nnls.py (solve_voxel_chi2) states it and the device output is
 * bit-identical.  Per voxel inside the mask, with finite samples:
 *   1  S(0) gives ss0;  yy = sum_i y_i^2, i ascending from 0.0.  Unless ss0 > exact_rel yy (an exact fit has no target):
 *      rule EXACT, the result is that of S(mu_exact), the weight mu_exact, the ratio 0.
 *   2  target = factor ss0, lo = 0, mu = mu_first.  For g = 0 .. n_grow: run S(mu); ss >= target is a hit and ends the
 *      loop (a NaN ss is none); else lo = mu and, if g < n_grow, mu = mu grow.  A hit at g == 0: rule LOW, the result is
 *      that of S(mu_first).  No hit: rule HIGH, the result is that of the last S run.
 *   3  Any other hit: hi = mu.  n_bisect times: mid = sqrt(lo hi), run S(mid), ss < target gives lo = mid, otherwise
 *      hi = mid.  The weight is sqrt(lo hi), the result that of S at it, rule FOUND.
 * x, func, amp and rmse are those of the final S;  mu_dev float32 of the weight;  ratio_dev float32 of ss_final / ss0 (0 for
 * EXACT);  solves_dev int32, the S runs above (2 for EXACT and LOW, n_grow + 2 for HIGH, g + n_bisect + 3 for FOUND);
 * nit_dev the sum of nit and status_dev the largest status over those runs;  rule_dev int32.  A voxel outside the mask or
 * with a non-finite sample: everything 0, status MASKED / NONFINITE, rule -1.
 *
 * The kernel is t2fit_nnls_dev's compiled a second time: same launch shape and LDS (t2fit_nnls_workgroup), same persistent
 * grid; a wave keeps its voxel through all its solves. */
#define T2FIT_NNLS_RULE_FOUND 0 /* the target was bracketed and bisected */
#define T2FIT_NNLS_RULE_EXACT 1 /* the unregularised fit is exact: mu_exact */
#define T2FIT_NNLS_RULE_LOW 2   /* mu_first exceeds the target already: mu_first */
#define T2FIT_NNLS_RULE_HIGH 3  /* the largest weight of the bracket stays below the target: that weight */

typedef struct t2fit_nnls_chi2_params {
    double factor;    /* 1.02: the misfit aimed at, over the unregularised one */
    double mu_first;  /* 1e-3: the first weight of the bracket */
    double grow;      /* 4: the bracket's growth per step */
    double exact_rel; /* 1e-12: ss0 <= exact_rel sum y^2 is an exact fit */
    double mu_exact;  /* 0.03: the weight of an exact fit */
    int32_t n_grow;   /* 6: growth steps at most (the bracket ends at mu_first grow^n_grow) */
    int32_t n_bisect; /* 5: bisections of the bracket, geometric */
} t2fit_nnls_chi2_params;

int t2fit_nnls_chi2_params_default(t2fit_nnls_chi2_params *chi2);

/* Arguments as t2fit_nnls_dev; mu_dev, ratio_dev float32 and solves_dev, rule_dev int32, [n_vox] each, are mandatory and
 * written for every voxel.  Refused before HIP is touched: everything t2fit_nnls_dev refuses, a NULL chi2 or new output
 * (or one not aligned to 4 bytes), a factor or grow that is not finite and above 1, a mu_first that is not finite and above
 * 0, an exact_rel or mu_exact that is negative or not finite, n_grow or n_bisect outside 0 .. 64.  After the header
 * read-back also a header whose mu is not 0: the rule owns the weight and the block's G must be A^T A. */
int t2fit_nnls_chi2_dev(const t2fit_nnls_params *params, const t2fit_nnls_chi2_params *chi2, const float *y_dev, int n_te,
                        int64_t n_vox, const uint8_t *mask_dev, const void *packed_dev, float *x_dev, float *func_dev,
                        float *amp_dev, float *rmse_dev, int32_t *nit_dev, int32_t *status_dev, float *mu_dev, float *ratio_dev,
                        int32_t *solves_dev, int32_t *rule_dev, void *stream);

/* Kernel timing for benchmarks (no reference counterpart).  With timing enabled (t2fit_set_timing(1)) every
 * t2fit_volume_dev call of this thread records HIP events around its fit kernel on the launch stream.
 * t2fit_kernel_ms(k): duration in milliseconds of the fit kernel launched k timed calls ago (0 = the most recent;
 * the last 16 are kept), waiting for that launch to finish if it has not; negative when unavailable.
 * t2fit_last_kernel_ms() = t2fit_kernel_ms(0).
 * t2fit_epilogue_ms(k): duration of the streaming epilogue pass (residual map, R^2, T2 standard error) that followed
 * that fit kernel; 0 for the one-pass kernels (closed form, one-shot LM), which have none. */
int t2fit_set_timing(int enabled);
double t2fit_kernel_ms(int launches_ago);
double t2fit_last_kernel_ms(void);
double t2fit_epilogue_ms(int launches_ago);

/* Multi-GPU tuning: the reference-trajectory fit is a persistent kernel whose resident workgroups hold all of every
 * CU's LDS, so a collective's kernel on another stream (RCCL's all-gather of the previous maps) may not become resident
 * before it drains.  `cus` > 0 launches the fit that many CUs' worth of workgroups short (costs cus/256 of its speed):
 * the chip then keeps that many workgroup slots -- their LDS and wave slots -- free; with the one-wave workgroups of the
 * large-volume kernels the dispatcher spreads them over the CUs of its choice (free slots, not whole CUs).  0 = use
 * everything (default; the environment variable T2FIT_RESERVE_CUS sets the initial value).  Process-wide, may be called
 * from any thread at any time (atomic); never changes a result.  Returns the previous setting.  No reference
 * counterpart (the reference is single-process). */
int t2fit_set_reserve_cus(int cus);

const char *t2fit_last_error(void);
int t2fit_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* T2FIT_H */
