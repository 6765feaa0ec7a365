"""Host-side mirror of the reference's fitting interface, backed by the HIP library.

Same names, argument meaning and error behaviour as the reference's hot path:

=============================  ================================================================
this module                    reference (paths relative to /root/reference)
=============================  ================================================================
``set_fit_params(args)``       run_t2mapping.py:29-111
``fit_voxel(...)``             run_t2mapping.py:120-312 (one voxel; same 5-tuple)
``fit_voxels(...)``            the ``Pool.map`` over ``fit_voxel`` (:430-443), batched
``stack_mask_flatten(...)``    run_t2mapping.py:383-386,411-421
``fit_volume(...)``            run_t2mapping.py:411-461 (flatten, fit, scatter, residual map)
``compute_residuals(...)``     utils/t2map_utils.py:62-89
=============================  ================================================================

Python here only marshals buffers; all arithmetic happens in libt2fit_hip.so through the C ABI of
include/t2fit.h.  torch is used for device buffers and streams, nothing else.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _abi
from ._lib import check, load, require_gpu

# scipy defaults that apply when a table omits an option (scipy.optimize._lbfgsb_py._minimize_lbfgsb)
_SCIPY_DEFAULTS = {"ftol": 2.2204460492503131e-09, "gtol": 1e-5, "eps": 1e-8, "maxfun": 15000,
                   "maxiter": 15000, "maxls": 20, "maxcor": 10}


# --------------------------------------------------------------------------------------------
# fit tables
# --------------------------------------------------------------------------------------------
def fit_table(fit: str, low_field: bool) -> dict:
    """The reference's ``fit_params`` dict for (fit, field), read from the library's tables."""
    cfg = _abi.T2FitConfig()
    check(load().t2fit_config_default(C.byref(cfg), _abi.MODELS[fit], int(bool(low_field))))
    n_par = 2 if fit == "gaussian" else 3

    def _num(v):  # the reference writes ints where it can; keep printing identical
        return int(v) if float(v).is_integer() else float(v)

    options = {"ftol": cfg.ftol, "maxls": cfg.maxls, "disp": False}
    if fit != "gaussian":
        options = {"gtol": cfg.gtol, "ftol": cfg.ftol, "maxls": cfg.maxls, "disp": False}
    return {
        "initial_guess": [_num(cfg.x0[j]) for j in range(n_par)],
        "param_bounds": [(_num(cfg.lb[j]), _num(cfg.ub[j])) for j in range(n_par)],
        "solver": "L-BFGS-B",
        "options": options,
    }


def set_fit_params(args):
    """run_t2mapping.py:29-111: ``args`` carries gaussian/gaussian_rician/rician, lf/hf, norm."""
    if getattr(args, "norm", False):
        print("Error: Normalization is set to true though no parameters where defined yet. "
              "Please modify set_fit_params to manage.")
        raise SystemExit(1)
    fit = "gaussian" if args.gaussian else "gaussian_rician" if args.gaussian_rician else "rician"
    if not (args.lf or args.hf):
        raise SystemExit(1)
    return fit, fit_table(fit, bool(args.lf))


def make_config(fit: str, fit_params: dict, TEeffs, prior: bool = True, norm: bool = False,
                solver: str = "lbfgsb", precision: str = "f64", numpy_legacy: bool = False) -> _abi.T2FitConfig:
    """Flatten (fit, fit_params, TEeffs, prior, norm) into the ABI struct.  ``numpy_legacy``: reproduce the reference
    as it runs under the numpy < 2 it freezes (requirements_frozen.txt:103) instead of under numpy >= 2: float32
    log term of the rician objective (run_t2mapping.py:169), float32 prediction of the residual map
    (utils/t2map_utils.py:74-80)."""
    if fit not in _abi.MODELS:
        raise ValueError(f"unknown fit {fit!r}")
    if fit_params.get("solver", "L-BFGS-B") != "L-BFGS-B":
        raise ValueError("only the reference's solver 'L-BFGS-B' is defined for fit_params['solver']")
    te = np.asarray(TEeffs, dtype=np.float64).ravel()
    if not 2 <= te.size <= _abi.MAX_TE:
        raise ValueError(f"need 2..{_abi.MAX_TE} echo times, got {te.size}")
    cfg = _abi.T2FitConfig()
    check(load().t2fit_config_default(C.byref(cfg), _abi.MODELS[fit], 1))
    n_par = 2 if fit == "gaussian" else 3
    x0 = list(fit_params["initial_guess"])
    bounds = list(fit_params["param_bounds"])
    if len(x0) != n_par:
        raise ValueError("length of initial_guess does not match the model")
    if len(bounds) != n_par:
        raise ValueError("length of x0 != length of bounds")  # scipy's message
    for j in range(3):
        cfg.x0[j] = float(x0[j]) if j < n_par else 0.0
        cfg.lb[j] = float(bounds[j][0]) if j < n_par else 0.0
        cfg.ub[j] = float(bounds[j][1]) if j < n_par else 0.0
    opts = dict(_SCIPY_DEFAULTS)
    opts.update({k: v for k, v in fit_params.get("options", {}).items() if k not in ("disp", "iprint")})
    if int(opts["maxcor"]) != 10:
        raise NotImplementedError("the lane solver keeps scipy's default maxcor=10 corrections")
    if not opts["maxls"] > 0:
        raise ValueError("maxls must be positive.")
    cfg.ftol, cfg.gtol, cfg.fd_step = float(opts["ftol"]), float(opts["gtol"]), float(opts["eps"])
    cfg.maxls, cfg.maxiter, cfg.maxfun = int(opts["maxls"]), int(opts["maxiter"]), int(opts["maxfun"])
    cfg.n_te = te.size
    for i in range(_abi.MAX_TE):
        cfg.te_ms[i] = float(te[i]) if i < te.size else 0.0
    cfg.no_prior = int(not prior)
    cfg.norm = int(bool(norm))
    cfg.numpy_legacy = int(bool(numpy_legacy))
    cfg.solver = _abi.SOLVERS[solver]
    cfg.precision = _abi.PRECISIONS[precision]
    if cfg.solver == _abi.SOLVER_LOGLIN and fit != "gaussian":
        raise ValueError("solver 'loglin' is the closed form of the 2-parameter 'gaussian' fit only")
    if cfg.solver == _abi.SOLVER_LM:
        cfg.maxiter = 0  # library default for LM
    return cfg


# --------------------------------------------------------------------------------------------
# stack / mask / flatten
# --------------------------------------------------------------------------------------------
def stack_mask_flatten(echo_vols: Sequence[np.ndarray], mask_vols: Sequence[np.ndarray], device: int = 0):
    """run_t2mapping.py:383-386,411-421 without the (Z,Y,X,nTE) transpose.

    Returns ``(echoes (nTE,N) float32 torch tensor on the GPU, mask (Z,Y,X) bool ndarray,
    mask_indices (M,) int64 ndarray)``; mask and indices are computed on the device and are
    bit-identical to ``np.sum(stack(masks),axis=3) > 0`` / ``np.where(...)[0]``.
    """
    import torch

    lib = require_gpu()
    shape = tuple(np.asarray(echo_vols[0]).shape)
    n = int(np.prod(shape))
    dev = torch.device("cuda", device)
    echoes = torch.empty((len(echo_vols), n), dtype=torch.float32, device=dev)
    for i, v in enumerate(echo_vols):
        echoes[i] = torch.from_numpy(np.ascontiguousarray(v).astype(np.float32, copy=False).reshape(-1)).to(dev)
    masks = torch.empty((len(mask_vols), n), dtype=torch.uint8, device=dev)
    for i, m in enumerate(mask_vols):
        masks[i] = torch.from_numpy((np.asarray(m) != 0).astype(np.uint8).reshape(-1)).to(dev)
    mask_d, idx_d, cnt_d = union_mask_dev(masks)
    count = int(cnt_d.item())
    return echoes, mask_d.cpu().numpy().astype(bool).reshape(shape), idx_d[:count].cpu().numpy()


def union_mask_dev(masks):
    """(n_masks, N) uint8 cuda tensor -> (mask uint8 [N], idx int64 [N] (first `count` valid), count)."""
    import torch

    lib = require_gpu()
    assert masks.is_cuda and masks.dtype == torch.uint8 and masks.is_contiguous() and masks.dim() == 2
    n = masks.shape[1]
    mask = torch.empty(n, dtype=torch.uint8, device=masks.device)
    idx = torch.empty(n, dtype=torch.int64, device=masks.device)
    cnt = torch.zeros(1, dtype=torch.int64, device=masks.device)
    with torch.cuda.device(masks.device):
        check(lib.t2fit_union_mask_dev(masks.data_ptr(), masks.shape[0], n, mask.data_ptr(), idx.data_ptr(),
                                       cnt.data_ptr(), _current_stream()))
    return mask, idx, cnt


def label_stats(map_, label, n_labels: int, device: int = 0):
    """Per-label ``(nanmean, nanstd, count)`` of a map on the GPU: the loop of ``save_phantom_csv``
    (utils/t2map_utils.py:43-53).  ``map_``: float32 array or CUDA tensor of any shape; ``label``: integer
    array/tensor of the same shape, vials numbered 1..n_labels.  Returns float64 / int64 numpy arrays."""
    import torch

    lib = require_gpu()
    dev = map_.device if type(map_).__module__.startswith("torch") and map_.is_cuda else torch.device("cuda", device)
    m = (map_ if type(map_).__module__.startswith("torch") else torch.from_numpy(np.ascontiguousarray(map_, np.float32)))
    m = m.to(dev, torch.float32).contiguous().reshape(-1)
    lab = label if type(label).__module__.startswith("torch") else torch.from_numpy(np.ascontiguousarray(label).astype(np.int32))
    lab = lab.to(dev, torch.int32).contiguous().reshape(-1)
    if lab.numel() != m.numel():
        raise ValueError("label shape does not match the map")
    mean = torch.empty(n_labels, dtype=torch.float64, device=dev)
    std = torch.empty(n_labels, dtype=torch.float64, device=dev)
    cnt = torch.empty(n_labels, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib.t2fit_label_stats_dev(m.data_ptr(), lab.data_ptr(), m.numel(), int(n_labels), mean.data_ptr(),
                                        std.data_ptr(), cnt.data_ptr(), _current_stream()))
    return mean.cpu().numpy(), std.cpu().numpy(), cnt.cpu().numpy()


# --------------------------------------------------------------------------------------------
# in-vivo atlas ROI statistics (utils/ada_utils.py:130-216 get_t2_per_roi, :885-968 compute_t2_per_tissue_feta)
# --------------------------------------------------------------------------------------------
ROI_MAX_LABELS = 256  # labels per library call (one 8-bit digit of its counting sort); more run in chunks here


@dataclass
class RoiStats:
    """Per-label statistics of one map, numpy arrays of length n_labels: ``mean`` / ``std`` (ddof = 0) / ``median``
    float64 over the non-NaN values (NaN for a label without any; ``median`` is None when it was not asked for),
    ``count`` int64 = voxels of the region (the reference's ``nvoxel``), ``valid`` int64 = those that are not NaN."""
    mean: np.ndarray
    std: np.ndarray
    median: Optional[np.ndarray]
    count: np.ndarray
    valid: np.ndarray


def _is_tensor(a) -> bool:
    return type(a).__module__.startswith("torch")


def _int_tensor(a):
    """An integer label volume (numpy array of any integer dtype, or a tensor) as a torch tensor, shape kept."""
    import torch

    if _is_tensor(a):
        if a.dtype.is_floating_point or a.dtype == torch.bool:
            raise ValueError("label volumes must have an integer dtype")
        return a
    a = np.asarray(a)
    if a.dtype.kind not in "iu":
        raise ValueError("label volumes must have an integer dtype")
    return torch.from_numpy(np.ascontiguousarray(a).astype(np.int64 if a.dtype.itemsize > 4 or a.dtype == np.uint32 else np.int32))


def dense_labels(label, labels):
    """Remap the label ids of interest to the dense range the kernels work on: voxels whose value is ``labels[i]``
    become ``i + 1``, every other voxel 0.  ``label``: integer torch tensor on any device (torch ops only, no copy to
    the host); ``labels``: distinct integer ids, e.g. the ``index`` values of an atlas XML or FreeSurfer ids.
    Returns an int32 tensor on the same device."""
    import torch

    ids = [int(v) for v in labels]
    if not ids:
        raise ValueError("labels is empty")
    if len(set(ids)) != len(ids):
        raise ValueError("labels holds an id twice")
    ids_t = torch.tensor(ids, dtype=torch.int64, device=label.device)
    sorted_ids, order = torch.sort(ids_t)
    lab = label.to(torch.int64)
    pos = torch.searchsorted(sorted_ids, lab.reshape(-1)).clamp_(max=len(ids) - 1).reshape(lab.shape)
    hit = sorted_ids[pos] == lab
    return torch.where(hit, order[pos] + 1, torch.zeros_like(pos)).to(torch.int32)


def _roi_device(arrays, device):
    import torch

    for a in arrays:
        if a is not None and _is_tensor(a) and a.is_cuda:
            return a.device
    return torch.device("cuda", device)


def roi_erode(label, tissue=None, tissue_value=None, *, labels=None, connectivity: int = 3, iterations: int = 1,
              device: int = 0):
    """The eroded region of every label at once: for each id ``L`` of ``labels`` the voxels of
    ``binary_erosion((tissue == tissue_value) & (label == L), generate_binary_structure(3, connectivity),
    iterations)`` (utils/ada_utils.py:165-169, :192-196, :925-933), as ONE int32 CUDA tensor shaped like ``label``
    that holds ``i + 1`` on the eroded region of ``labels[i]`` and 0 elsewhere (the masks of one atlas are disjoint).
    ``label`` / ``tissue``: 3-D numpy arrays or tensors of any integer dtype; ``labels`` defaults to
    ``1..label.max()``; ``iterations = 0`` returns the regions as they are."""
    import torch

    lib = require_gpu()
    dev = _roi_device((label, tissue), device)
    lab = _int_tensor(label)
    if lab.dim() != 3:
        raise ValueError("label must be a 3-D volume (z, y, x)")
    lab = lab.to(dev)
    tis = None
    if tissue is not None:
        if tissue_value is None:
            raise ValueError("tissue_value is required with tissue")
        tis = _int_tensor(tissue)
        if tuple(tis.shape) != tuple(lab.shape):
            raise ValueError("tissue shape does not match the label volume")
        tv = int(tissue_value)
        # the library compares int32 values: a wider tissue volume is reduced to {0, 1} first
        if tis.dtype in (torch.int64,) or not -2**31 <= tv < 2**31:
            tis, tv = (tis.to(dev) == tv).to(torch.int32), 1
        tis = tis.to(dev, torch.int32).contiguous()
    if labels is not None:
        lab, n = dense_labels(lab, labels), len(list(labels))
    else:
        n = max(int(lab.max().item()) if lab.numel() else 0, 1)
        lab = torch.where((lab >= 1) & (lab <= n), lab, torch.zeros_like(lab)).to(torch.int32)
    lab = lab.contiguous()
    nz, ny, nx = (int(v) for v in lab.shape)
    out = torch.empty_like(lab)
    with torch.cuda.device(dev):
        st = _current_stream()
        if n <= ROI_MAX_LABELS:
            check(lib.t2fit_roi_erode_dev(lab.data_ptr(), tis.data_ptr() if tis is not None else None,
                                          tv if tis is not None else 0, nz, ny, nx, n, int(connectivity), int(iterations),
                                          out.data_ptr(), st))
            return out
        out.zero_()
        part = torch.empty_like(lab)
        for lo in range(0, n, ROI_MAX_LABELS):  # chunks of 256 labels: the regions are disjoint, the results add up
            m = min(ROI_MAX_LABELS, n - lo)
            chunk = torch.where((lab > lo) & (lab <= lo + m), lab - lo, torch.zeros_like(lab)).contiguous()
            check(lib.t2fit_roi_erode_dev(chunk.data_ptr(), tis.data_ptr() if tis is not None else None,
                                          tv if tis is not None else 0, nz, ny, nx, m, int(connectivity), int(iterations),
                                          part.data_ptr(), st))
            out += torch.where(part > 0, part + lo, torch.zeros_like(part))
    return out


def roi_stats(map_, roi, n_labels: int, *, median: bool = True, device: int = 0) -> RoiStats:
    """``np.mean`` / ``np.std`` / ``np.median`` / ``len`` of ``map_[roi == L]`` for L in 1..n_labels on the GPU
    (utils/ada_utils.py:171-189).  ``map_``: float32 numpy array or CUDA tensor; ``roi``: integer array / tensor of the
    same shape, e.g. what :func:`roi_erode` returned.  NaN map values are left out and show as ``valid < count``."""
    import torch

    lib = require_gpu()
    n_labels = int(n_labels)
    if n_labels < 1:
        raise ValueError("n_labels must be at least 1")
    dev = _roi_device((map_, roi), device)
    m = map_ if _is_tensor(map_) else torch.from_numpy(np.ascontiguousarray(map_, np.float32))
    r = _int_tensor(roi)
    if tuple(m.shape) != tuple(r.shape):
        raise ValueError("roi shape does not match the map")
    m = m.to(dev, torch.float32).contiguous().reshape(-1)
    r = r.to(dev)
    if r.dtype != torch.int32:
        r = torch.where((r >= 1) & (r <= n_labels), r, torch.zeros_like(r)).to(torch.int32)
    r = r.contiguous().reshape(-1)
    mean = torch.empty(n_labels, dtype=torch.float64, device=dev)
    std = torch.empty(n_labels, dtype=torch.float64, device=dev)
    med = torch.empty(n_labels, dtype=torch.float64, device=dev) if median else None
    cnt = torch.empty(n_labels, dtype=torch.int64, device=dev)
    val = torch.empty(n_labels, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        st = _current_stream()
        for lo in range(0, n_labels, ROI_MAX_LABELS):
            k = min(ROI_MAX_LABELS, n_labels - lo)
            rc = r if n_labels <= ROI_MAX_LABELS else torch.where((r > lo) & (r <= lo + k), r - lo, torch.zeros_like(r)).contiguous()
            check(lib.t2fit_roi_stats_dev(m.data_ptr(), rc.data_ptr(), m.numel(), k, mean[lo:].data_ptr(), std[lo:].data_ptr(),
                                          med[lo:].data_ptr() if median else None, cnt[lo:].data_ptr(), val[lo:].data_ptr(), st))
    return RoiStats(mean.cpu().numpy(), std.cpu().numpy(), med.cpu().numpy() if median else None, cnt.cpu().numpy(),
                    val.cpu().numpy())


def roi_frame(index, names, count, valid, stats: dict):
    """The table :func:`roi_table` returns, from statistics that are already computed: ``stats`` maps a map's name to
    ``(mean, std, median)``.  ``np.mean`` / ``np.std`` / ``np.median`` of a float32 map are float32 numbers, so the
    statistics are rounded to float32 (and stored as float64, as ``phantom_frame`` does): the text pandas writes then
    has the digits numpy returns on the float32 map."""
    import pandas as pd

    index = [int(v) for v in index]
    names = [str(v) for v in (names if names is not None else index)]
    if len(names) != len(index):
        raise ValueError("names and labels differ in length")
    cols = {"roi": names, "index": index, "nvoxel": np.asarray(count, np.int64), "nvalid": np.asarray(valid, np.int64)}
    for m, (mean, std, med) in stats.items():
        for stat, v in (("mean", mean), ("std", std), ("median", med)):
            cols[f"{stat}_{m}"] = np.asarray(v, np.float64).astype(np.float32).astype(np.float64)
    return pd.DataFrame(cols)


def roi_table(maps: dict, label, tissue=None, tissue_value=None, *, labels=None, names=None, connectivity: int = 3,
              iterations: int = 1, device: int = 0):
    """``get_t2_per_roi`` for one atlas (utils/ada_utils.py:130-216) as a ``pandas.DataFrame``: the regions are eroded
    once (:func:`roi_erode`), then every map of ``maps`` (name -> float32 volume) is reduced per region
    (:func:`roi_stats`).  One row per id of ``labels`` (default ``1..label.max()``); columns ``roi`` (``names[i]``, the
    id when there are none), ``index`` (the id), ``nvoxel``, ``nvalid``, then ``mean_<m>``, ``std_<m>``, ``median_<m>``
    per map."""
    if not maps:
        raise ValueError("maps is empty")
    roi = roi_erode(label, tissue, tissue_value, labels=labels, connectivity=connectivity, iterations=iterations, device=device)
    if labels is not None:
        index = [int(v) for v in labels]
    else:
        lab = _int_tensor(label)
        index = list(range(1, max(int(lab.max().item()) if lab.numel() else 0, 1) + 1))
    count = valid = None
    stats = {}
    for name, m in maps.items():
        if tuple(m.shape) != tuple(roi.shape):
            raise ValueError(f"map {name!r} does not have the label volume's shape")
        s = roi_stats(m, roi, len(index), device=device)
        stats[name] = (s.mean, s.std, s.median)
        # nvoxel is the same for every map; nvalid is the first map's (the maps of one fit are NaN in the same voxels)
        count, valid = (s.count, s.valid) if count is None else (count, valid)
    return roi_frame(index, names, count, valid, stats)


# --------------------------------------------------------------------------------------------
# volume seam
# --------------------------------------------------------------------------------------------
@dataclass
class T2Maps:
    """The reference's four maps (utils/t2map_utils.py:18-29) plus optional per-voxel extras."""
    t2: object
    k: object
    sigma: object
    res: object
    r2: Optional[object] = None
    fun: Optional[object] = None
    nit: Optional[object] = None
    status: Optional[object] = None
    t2_se: Optional[object] = None  # standard error of T2 (extension; 95 % CI = T2 +- 1.96 t2_se)

    def success(self):
        """scipy ``result.success`` per voxel (False outside the mask)."""
        return None if self.status is None else (self.status == _abi.ST_CONVERGED)


def _layout_of(echoes_shape, n_te, layout):
    if layout in ("te_major", _abi.LAYOUT_TE_MAJOR):
        if echoes_shape[0] != n_te:
            raise ValueError(f"te_major echoes need shape (nTE, ...): got {tuple(echoes_shape)} for nTE={n_te}")
        return _abi.LAYOUT_TE_MAJOR, tuple(echoes_shape[1:])
    if layout in ("voxel_major", _abi.LAYOUT_VOXEL_MAJOR):
        if echoes_shape[-1] != n_te:
            raise ValueError(f"voxel_major echoes need shape (..., nTE): got {tuple(echoes_shape)} for nTE={n_te}")
        return _abi.LAYOUT_VOXEL_MAJOR, tuple(echoes_shape[:-1])
    raise ValueError(f"unknown layout {layout!r}")


def fit_volume(echoes, mask, TEeffs, fit, fit_params, prior=True, norm=False, *, layout="te_major",
               solver="lbfgsb", precision="f64", extras=False, strict=True, device=0, out: T2Maps = None,
               numpy_legacy=False):
    """Fit every masked voxel and return the maps (run_t2mapping.py:411-461).

    ``echoes``: float32 ``(nTE, Z, Y, X)`` (``layout='te_major'``, the per-TE volumes as read) or
    ``(Z, Y, X, nTE)`` (``'voxel_major'``, the reference's ``t2w``); numpy array or CUDA torch tensor.
    ``mask``: same spatial shape, non-zero = fit, or None.  Returns :class:`T2Maps` shaped ``(Z,Y,X)``
    -- numpy for numpy input (host entry point), torch for torch input (device entry point,
    asynchronous on the current stream).  ``strict``: raise ValueError, as the reference's scipy call
    does, if a voxel's data-dependent bounds are infeasible (numpy path; the torch path never syncs).
    """
    cfg = make_config(fit, fit_params, TEeffs, prior, norm, solver, precision, numpy_legacy)
    lib = require_gpu()
    lay, spatial = _layout_of(echoes.shape, cfg.n_te, layout)
    n = int(np.prod(spatial)) if len(spatial) else 1
    is_torch = type(echoes).__module__.startswith("torch")
    maps = _abi.T2FitMaps()
    if is_torch:
        import torch

        if not (echoes.is_cuda and echoes.dtype == torch.float32 and echoes.is_contiguous()):
            raise ValueError("torch echoes must be a contiguous float32 CUDA tensor")
        dev = echoes.device
        if mask is not None:
            if not (mask.is_cuda and mask.dtype == torch.uint8 and mask.is_contiguous() and mask.numel() == n):
                raise ValueError("torch mask must be a contiguous uint8 CUDA tensor of the spatial shape")
        if out is None:
            f32 = lambda: torch.empty(spatial, dtype=torch.float32, device=dev)  # noqa: E731
            out = T2Maps(f32(), f32(), f32(), f32())
            if extras:
                out.r2, out.fun, out.t2_se = f32(), f32(), f32()
                out.nit = torch.empty(spatial, dtype=torch.int32, device=dev)
                out.status = torch.empty(spatial, dtype=torch.uint8, device=dev)
        for name in ("t2", "k", "sigma", "res", "r2", "fun", "nit", "status", "t2_se"):
            t = getattr(out, name)
            if t is not None:  # the library writes raw bytes of this type through the pointer: check before it does
                want = {"nit": torch.int32, "status": torch.uint8}.get(name, torch.float32)
                if not (torch.is_tensor(t) and t.dtype == want and t.device == dev and t.is_contiguous() and t.numel() == n):
                    raise ValueError(f"out.{name} must be a contiguous {str(want).split('.')[-1]} tensor on {dev} with {n} elements")
            elif name in ("t2", "k", "sigma", "res"):
                raise ValueError(f"out.{name} is required")
            setattr(maps, name, None if t is None else t.data_ptr())
        with torch.cuda.device(dev):
            check(lib.t2fit_volume_dev(C.byref(cfg), echoes.data_ptr(), lay,
                                       None if mask is None else mask.data_ptr(), n, C.byref(maps),
                                       _current_stream()))
        return out
    e = np.ascontiguousarray(echoes, dtype=np.float32)
    m = None
    if mask is not None:
        m = np.asarray(mask)
        # the kernels test mask != 0 themselves: one-byte masks go in as they are
        m = np.ascontiguousarray(m).view(np.uint8) if m.dtype.itemsize == 1 else np.ascontiguousarray(m != 0, dtype=np.uint8)
        if m.size != n:
            raise ValueError("mask shape does not match the echoes")
    if out is None:  # (callers that fit one volume after the other may hand the previous T2Maps back in as `out`)
        f32 = lambda: _new_map(spatial, np.float32)  # noqa: E731
        out = T2Maps(f32(), f32(), f32(), f32())
        if extras:
            out.r2, out.fun, out.nit, out.t2_se = f32(), f32(), _new_map(spatial, np.int32), f32()
    want_status = out.status is not None
    if out.status is None:
        out.status = _new_map(spatial, np.uint8)
    for name in ("t2", "k", "sigma", "res", "r2", "fun", "nit", "status", "t2_se"):
        a = getattr(out, name)
        want = {"nit": np.int32, "status": np.uint8}.get(name, np.float32)  # what the library writes through the pointer
        if a is not None and not (isinstance(a, np.ndarray) and a.dtype == want and a.flags.c_contiguous
                                  and a.flags.writeable and a.size == n):
            raise ValueError(f"out.{name} must be a writable C-contiguous {np.dtype(want).name} numpy array with {n} elements")
        if a is None and name in ("t2", "k", "sigma", "res"):
            raise ValueError(f"out.{name} is required")
        setattr(maps, name, None if a is None else a.ctypes.data)
    check(lib.t2fit_volume_host(C.byref(cfg), e.ctypes.data, lay, None if m is None else m.ctypes.data, n,
                                C.byref(maps), int(device)))
    if strict and np.any(out.status == _abi.ST_INFEASIBLE):
        bad = int(np.flatnonzero(out.status.reshape(-1) == _abi.ST_INFEASIBLE)[0])
        raise ValueError("LBFGSB - one of the lower bounds is greater than an upper bound. "
                         f"(voxel {bad}: S(TE0) exceeds the no-prior upper bound)")
    if not extras and not want_status:
        out.status = None
    return out


_libc = None


def _new_map(shape, dtype):
    """A fresh output array.  Large ones are advised to use transparent huge pages: the library's copy threads touch
    every page of a new map for the first time, and 67 MB in 4 KiB pages are 16 384 page faults per map and call."""
    global _libc
    a = np.empty(shape, dtype)
    if a.nbytes >= (8 << 20):
        try:
            if _libc is None:
                _libc = C.CDLL(None, use_errno=True)
            huge = 2 << 20
            lo = (a.ctypes.data + huge - 1) & ~(huge - 1)
            hi = (a.ctypes.data + a.nbytes) & ~(huge - 1)
            if hi > lo:
                _libc.madvise(C.c_void_p(lo), C.c_size_t(hi - lo), 14)  # MADV_HUGEPAGE; failure is harmless
        except (OSError, AttributeError):
            pass
    return a


# --------------------------------------------------------------------------------------------
# voxel seam
# --------------------------------------------------------------------------------------------
def fit_voxels(indices, fit, fit_params, TEeffs, reshaped_t2w, prior, norm, *, solver="lbfgsb",
               precision="f64", device=0, numpy_legacy=False):
    """Batched ``fit_voxel``: rows ``indices`` of the (N, nTE) float32 stack.

    Returns ``(x (M,n_par) f64, success (M,) bool, nit (M,) int32, fun (M,) f64, status (M,) u8)``.
    """
    cfg = make_config(fit, fit_params, TEeffs, prior, norm, solver, precision, numpy_legacy)
    lib = require_gpu()
    data = np.ascontiguousarray(reshaped_t2w, dtype=np.float32)
    if data.ndim != 2 or data.shape[1] != cfg.n_te:
        raise ValueError("reshaped_t2w must be (N, nTE)")
    idx = np.ascontiguousarray(np.atleast_1d(indices), dtype=np.int64)
    m = idx.size
    x = np.zeros((m, 3))
    fun = np.zeros(m)
    nit = np.zeros(m, np.int32)
    st = np.zeros(m, np.uint8)
    check(lib.t2fit_voxels_host(C.byref(cfg), data.ctypes.data, _abi.LAYOUT_VOXEL_MAJOR, data.shape[0],
                                idx.ctypes.data, m, x.ctypes.data, fun.ctypes.data, nit.ctypes.data,
                                st.ctypes.data, int(device)))
    n_par = 2 if fit == "gaussian" else 3
    return x[:, :n_par], st == _abi.ST_CONVERGED, nit, fun, st


def fit_voxels_trace(indices, fit, fit_params, TEeffs, reshaped_t2w, prior, norm, *, trace_cap=64, solver="lbfgsb",
                     precision="f64", device=0, numpy_legacy=False):
    """``fit_voxels`` plus, per voxel, the reference's ``iteration_info`` (run_t2mapping.py:180-234): a
    list of ``{'f_val', 'grad_norm': None, 'step_size'}`` dicts, one per iteration (at most ``trace_cap``)."""
    cfg = make_config(fit, fit_params, TEeffs, prior, norm, solver, precision, numpy_legacy)
    lib = require_gpu()
    data = np.ascontiguousarray(reshaped_t2w, dtype=np.float32)
    idx = np.ascontiguousarray(np.atleast_1d(indices), dtype=np.int64)
    m = idx.size
    x, fun = np.zeros((m, 3)), np.zeros(m)
    nit, st = np.zeros(m, np.int32), np.zeros(m, np.uint8)
    tr, tl = np.zeros((m, trace_cap, 4)), np.zeros(m, np.int32)
    check(lib.t2fit_voxels_trace_host(C.byref(cfg), data.ctypes.data, _abi.LAYOUT_VOXEL_MAJOR, data.shape[0],
                                      idx.ctypes.data, m, x.ctypes.data, fun.ctypes.data, nit.ctypes.data,
                                      st.ctypes.data, int(trace_cap), tr.ctypes.data, tl.ctypes.data, int(device)))
    n_par = 2 if fit == "gaussian" else 3
    infos = []
    for r in range(m):
        pts = tr[r, : tl[r]]
        steps = np.r_[np.nan, np.linalg.norm(np.diff(pts[:, :n_par], axis=0), axis=1)] if len(pts) else []
        infos.append([{"f_val": float(p[3]), "grad_norm": None, "step_size": float(s)} for p, s in zip(pts, steps)])
    return x[:, :n_par], st == _abi.ST_CONVERGED, nit, fun, st, infos


def fit_voxel(voxel, fit, fit_params, TEeffs, reshaped_t2w, prior, norm, want_trace=True, **kw):
    """run_t2mapping.py:120-312 for one voxel: ``(params, success, nit, final_error, iteration_info)``.

    Like the reference, a voxel whose no-prior bounds are infeasible raises ValueError, and
    ``fit_params['param_bounds']`` is rewritten in place when ``prior`` is False (:243-245).
    ``iteration_info`` holds the objective value and step length of every iteration, as the
    reference's callbacks record them.
    """
    if not prior:
        fit_params["param_bounds"][0] = (reshaped_t2w[voxel, 0], 10000)
        fit_params["param_bounds"][1] = (10, 2000)
        if fit_params["param_bounds"][0][0] > 10000:
            raise ValueError("LBFGSB - one of the lower bounds is greater than an upper bound.")
    if want_trace:
        x, ok, nit, fun, st, infos = fit_voxels_trace([voxel], fit, fit_params, TEeffs, reshaped_t2w, prior, norm, **kw)
    else:
        x, ok, nit, fun, st = fit_voxels([voxel], fit, fit_params, TEeffs, reshaped_t2w, prior, norm, **kw)
        infos = [[]]
    if not ok[0]:
        print(f"FAIL : Optimization failed for voxel {voxel}: status {int(st[0])}")
        print("Objective function value at optimum:", fun[0])
        print("params", x[0])
    return x[0], bool(ok[0]), int(nit[0]), float(fun[0]), infos[0]


# --------------------------------------------------------------------------------------------
# residual map
# --------------------------------------------------------------------------------------------
def compute_residuals(reshaped_t2w, TEeffs, fit, norm, k_map, t2_map, sigma_map, res_map, mask_indices, mask,
                      device=0, numpy_legacy=False):
    """utils/t2map_utils.py:62-89 with the reference's signature; evaluated on the GPU."""
    import torch

    lib = require_gpu()
    data = np.ascontiguousarray(reshaped_t2w, dtype=np.float32)
    n, n_te = data.shape
    cfg = make_config(fit, fit_table(fit, True), TEeffs, True, norm, numpy_legacy=numpy_legacy)
    dev = torch.device("cuda", device)
    e = torch.from_numpy(data).to(dev)
    sel = torch.zeros(n, dtype=torch.uint8, device=dev)
    sel[torch.from_numpy(np.asarray(mask_indices, dtype=np.int64)).to(dev)] = 1
    t2 = torch.from_numpy(np.ascontiguousarray(t2_map, np.float32).reshape(-1)).to(dev)
    k = torch.from_numpy(np.ascontiguousarray(k_map, np.float32).reshape(-1)).to(dev)
    sg = torch.from_numpy(np.ascontiguousarray(sigma_map, np.float32).reshape(-1)).to(dev)
    res = torch.empty(n, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.t2fit_residuals_dev(C.byref(cfg), e.data_ptr(), _abi.LAYOUT_VOXEL_MAJOR, sel.data_ptr(), n,
                                      t2.data_ptr(), k.data_ptr(), sg.data_ptr(), res.data_ptr(), _current_stream()))
    out = np.asarray(res_map, dtype=np.float32).reshape(-1).copy()
    r = res.cpu().numpy()
    mi = np.asarray(mask_indices, dtype=np.int64)
    out[mi] = r[mi]
    return out.reshape(np.asarray(mask).shape[:3])


# --------------------------------------------------------------------------------------------
# parametric bootstrap (no reference counterpart): how far to trust a fitted value
# --------------------------------------------------------------------------------------------
@dataclass
class BootStats:
    """Bootstrap maps of one parameter, ``(Z, Y, X)`` float32: ``mean`` of the counted replicas, ``bias`` = mean - the
    fitted value, ``std`` (ddof = 1, NaN when fewer than two replicas count), ``ci_lo`` / ``ci_hi`` = numpy's default
    percentiles at 100 alpha / 2 and 100 (1 - alpha / 2) (None when no interval was asked for).  Zeros outside the mask."""
    mean: object
    bias: object
    std: object
    ci_lo: Optional[object] = None
    ci_hi: Optional[object] = None


@dataclass
class BootMaps:
    """What :func:`bootstrap_volume` returns: one :class:`BootStats` per requested parameter (None otherwise), ``n_ok``
    (int32: replicas of the voxel that count -- the refit converged and its values are finite), the fit the replicas
    were drawn from (``fit``: :class:`T2Maps`) and the settings: ``noise_sigma`` (the number used, None for a map),
    ``n_replicas``, ``seed``, ``alpha``."""
    t2: Optional[BootStats]
    k: Optional[BootStats]
    sigma: Optional[BootStats]
    n_ok: object
    fit: T2Maps
    noise_sigma: Optional[float]
    n_replicas: int
    seed: int
    alpha: float

    # the T2 maps under the names the documentation uses
    boot_mean = property(lambda self: self.t2.mean)
    boot_bias = property(lambda self: self.t2.bias)
    boot_std = property(lambda self: self.t2.std)
    ci_lo = property(lambda self: self.t2.ci_lo)
    ci_hi = property(lambda self: self.t2.ci_hi)


def _f32_dev(a, dev, n=None, what="array"):
    """numpy array or tensor -> contiguous flat float32 tensor on `dev`."""
    import torch

    t = a if _is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))
    t = t.to(dev, torch.float32).contiguous().reshape(-1)
    if n is not None and t.numel() != n:
        raise ValueError(f"{what} has {t.numel()} elements, the volume has {n}")
    return t


def _mask_dev(mask, dev, n):
    import torch

    if mask is None:
        return torch.ones(n, dtype=torch.uint8, device=dev)
    m = mask if _is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0).view(np.uint8))
    m = (m != 0).to(dev, torch.uint8).contiguous().reshape(-1)
    if m.numel() != n:
        raise ValueError("mask shape does not match the volume")
    return m


_BOOT_SYMBOLS, _TV_SYMBOLS, _RECON_SYMBOLS = _abi.ADDITIVE[0:3], _abi.ADDITIVE[3:6], _abi.ADDITIVE[6:9]


def _require(*symbols):
    """The library, with these entry points (additive symbols of ABI 5: looked up, not assumed)."""
    lib = require_gpu()
    missing = [name for name in symbols if not hasattr(lib, name)]
    if missing:
        raise RuntimeError(f"this build of libt2fit_hip.so lacks {', '.join(missing)}: rebuild it "
                           "(python -m fetal_t2mapping_amd.build)")
    return lib


def _current_stream():
    """The current device's current torch stream, as the C ABI takes one."""
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _workspace(nbytes, dev):
    """A device workspace of nbytes for the library: the tensor that owns it and the pointer, 256-byte aligned."""
    import torch

    ws = torch.empty(nbytes + 256, dtype=torch.uint8, device=dev)
    return ws, (ws.data_ptr() + 255) // 256 * 256


def _noise_kind(noise):
    if noise not in _abi.BOOT_NOISES:
        raise ValueError(f"noise must be 'rician' or 'gaussian', got {noise!r}")
    return _abi.BOOT_NOISES[noise]


def estimate_background_sigma(echoes, mask, *, layout="te_major", device=0):
    """Noise level from the background: ``sqrt(sum(S**2) / (2 M))`` over the ``M`` samples (all echoes) of the voxels
    outside ``mask`` -- the second moment of the Rayleigh distribution of a magnitude image without signal.  float64 on
    the GPU with a fixed summation tree (the same bits from call to call).  ``echoes`` as in :func:`fit_volume`.
    Returns ``(sigma, M)``; a mask that covers everything raises ValueError."""
    import torch

    lib = _require(*_BOOT_SYMBOLS)
    if mask is None:
        raise ValueError("estimate_background_sigma needs a mask: the noise is measured outside it")
    n_te = int(echoes.shape[0] if layout in ("te_major", _abi.LAYOUT_TE_MAJOR) else echoes.shape[-1])
    lay, spatial = _layout_of(echoes.shape, n_te, layout)
    n = int(np.prod(spatial)) if len(spatial) else 1
    dev = _roi_device((echoes, mask), device)
    e = _f32_dev(echoes, dev)
    m = _mask_dev(mask, dev, n)
    sigma, count = C.c_double(0.0), C.c_int64(0)
    with torch.cuda.device(dev):
        check(lib.t2fit_boot_background_dev(e.data_ptr(), lay, m.data_ptr(), n_te, n, C.byref(sigma), C.byref(count),
                                            _current_stream()))
    return float(sigma.value), int(count.value)


def tv_params(weight=0.1, eps=2e-4, max_iter=200, dims=2, precision="f32"):
    """The POD of :func:`denoise_tv` (``t2fit_tv_params``); the library checks the values."""
    if precision not in _abi.PRECISIONS:
        raise ValueError(f"precision must be 'f32' or 'f64', got {precision!r}")
    return _abi.T2FitTvParams(float(weight), float(eps), int(max_iter), int(dims), _abi.PRECISIONS[precision], 0)


def denoise_tv(echoes, weight=0.1, *, eps=2e-4, max_iter=200, dims=2, precision="f32", out=None, return_info=False,
               layout="te_major", device=0, max_workspace_bytes=None):
    """Total-variation denoising of the echo stack on the GPU by Chambolle's projection algorithm, as scikit-image
    0.22's ``denoise_tv_chambolle`` defines it on a float image: what the reference's ``run_denoising`` does to every
    slice of every echo before the fit reads them (utils/qmri_utils.py:393-405; ``weight``, ``eps``, ``max_iter``
    default to skimage's).  ``weight`` is in intensity units of the stack.

    ``echoes``: float32 ``(Z, Y, X)`` or ``(n, Z, Y, X)``, numpy array (numpy result) or CUDA tensor (tensor result,
    asynchronous on the current stream).  ``dims=2``: every ``(Y, X)`` slice is a problem (the reference's), ``dims=3``:
    every volume.  ``precision='f32'`` iterates in float32, ``'f64'`` in float64 with one rounding at the end.
    ``out``: a float32 CUDA tensor of the stack's shape to write into (may be ``echoes`` itself); tensor input only.
    ``return_info``: also return ``{'n_iter': int32 per problem, 'energy': float64 per problem}`` (problems in memory
    order: ``n * Z`` slices or ``n`` volumes).  The workspace is a torch buffer; when it would not fit into the free
    device memory (or ``max_workspace_bytes``) the volumes are run in groups, which changes no result.
    :mod:`fetal_t2mapping_amd._tv` states the same loop in numpy."""
    import torch

    lib = _require(*_TV_SYMBOLS)
    if layout in ("voxel_major", _abi.LAYOUT_VOXEL_MAJOR):
        raise ValueError("denoise_tv takes the te-major stack (nTE, Z, Y, X): a slice must be contiguous.  Permute a "
                         "voxel-major (Z, Y, X, nTE) stack first: np.moveaxis(echoes, -1, 0) or echoes.permute(3, 0, 1, 2)")
    if layout not in ("te_major", _abi.LAYOUT_TE_MAJOR):
        raise ValueError(f"unknown layout {layout!r}")
    shape = tuple(int(v) for v in echoes.shape)
    if len(shape) not in (3, 4):
        raise ValueError(f"denoise_tv needs a (Z, Y, X) volume or an (n, Z, Y, X) stack, got shape {shape}")
    n_vol = shape[0] if len(shape) == 4 else 1
    nz, ny, nx = shape[-3:]
    par = tv_params(weight, eps, max_iter, dims, precision)
    is_t = _is_tensor(echoes)
    if out is not None and not is_t:
        raise ValueError("out= goes with a CUDA tensor input (a numpy input returns a new array)")
    need = C.c_size_t(0)
    check(lib.t2fit_tv_workspace_bytes(C.byref(par), n_vol, nz, ny, nx, C.byref(need)))
    dev = _roi_device((echoes,), device)
    src = _f32_dev(echoes, dev)
    if out is None:
        dst = torch.empty_like(src)
    else:
        if not (_is_tensor(out) and out.is_cuda and out.dtype == torch.float32 and out.is_contiguous()
                and tuple(out.shape) == shape and out.device == src.device):
            raise ValueError("out must be a contiguous float32 CUDA tensor of the stack's shape on the stack's device")
        dst = out.reshape(-1)
    n_prob_vol = nz if par.dims == 2 else 1
    n_iter = torch.empty(n_vol * n_prob_vol, dtype=torch.int32, device=dev)
    energy = torch.empty(n_vol * n_prob_vol, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        budget = int(torch.cuda.mem_get_info(dev)[0] * 0.9) if max_workspace_bytes is None else int(max_workspace_bytes)
        group = n_vol
        while group > 1 and need.value > budget:
            group = (group + 1) // 2
            check(lib.t2fit_tv_workspace_bytes(C.byref(par), group, nz, ny, nx, C.byref(need)))
        ws, ws_ptr = _workspace(need.value, dev)
        stream = _current_stream()
        n_v = nz * ny * nx
        for v0 in range(0, n_vol, group):
            g = min(group, n_vol - v0)
            check(lib.t2fit_tv_denoise_dev(C.byref(par), src.data_ptr() + 4 * v0 * n_v, dst.data_ptr() + 4 * v0 * n_v, g, nz,
                                           ny, nx, ws_ptr, need.value, n_iter.data_ptr() + 4 * v0 * n_prob_vol,
                                           energy.data_ptr() + 8 * v0 * n_prob_vol, stream))
        ws.record_stream(torch.cuda.current_stream())
    res = dst.reshape(shape)
    if not is_t:
        res = res.cpu().numpy()
    if not return_info:
        return res
    info = {"n_iter": n_iter, "energy": energy}
    if not is_t:
        info = {k: v.cpu().numpy() for k, v in info.items()}
    return res, info


def _geometry_header(g):
    """A grid as a ``nifti.Image`` over an empty array: spacing / origin / direction for the writer."""
    from . import nifti

    return nifti.Image(np.zeros((0, 0, 0), np.float32), g.GetSpacing(), g.GetOrigin(), g.GetDirection())


def resample_volume(vol, geom, *, res=None, like=None, transform=None, interp="linear", default=0.0, integer_cast=False,
                    device=0):
    """Resample ``vol`` -- ``(Z, Y, X)`` or ``(n, Z, Y, X)`` volumes that share the geometry ``geom`` (anything with
    GetSpacing / GetOrigin / GetDirection: a ``nifti.Image``) -- on the GPU.  The output grid is ``geom`` at ``res`` mm
    isotropic (the reference's ``resample_volume``, utils/qmri_utils.py:62-80; the default with ``res=1.0``) or the grid
    ``like`` (anything with the four Get* methods including GetSize, e.g. a :class:`_resample.Geometry`).  ``transform``:
    4 x 4, maps a physical point of the output grid to a physical point of ``vol`` (``sitk.Resample``'s sense).
    ``interp='linear'`` takes float32 and returns float32; ``'nearest'`` copies float32 or int32 (label / mask volumes).
    ``integer_cast``: truncate toward zero and clamp to int16's range, as a stack that keeps an int16 pixel type does.
    numpy in, numpy out; CUDA tensor in, tensor out (asynchronous on the current stream).  Returns ``(out, geometry)``.
    :mod:`fetal_t2mapping_amd._resample` states the definition in numpy; the result is bit-identical to it."""
    import torch

    from . import _resample

    lib = _require(*_RECON_SYMBOLS)
    if interp not in _abi.INTERPS:
        raise ValueError(f"interp must be 'linear' or 'nearest', got {interp!r}")
    if (res is None) == (like is None):
        if like is not None:
            raise ValueError("give res= or like=, not both")
        res = 1.0
    shape = tuple(int(v) for v in vol.shape)
    if len(shape) not in (3, 4):
        raise ValueError(f"resample_volume needs a (Z, Y, X) volume or an (n, Z, Y, X) stack, got shape {shape}")
    n_vol = shape[0] if len(shape) == 4 else 1
    src_geom = _resample.as_geometry(geom, shape[-3:])
    dst_geom = _resample.isotropic_geometry(src_geom, res) if like is None else _resample.as_geometry(like)
    A = _resample.index_affine(dst_geom, src_geom, transform)
    is_t = _is_tensor(vol)
    dev = _roi_device((vol,), device)
    as_int = (vol.dtype in (torch.int32, torch.int16, torch.uint8, torch.int8)) if is_t else (np.asarray(vol).dtype.kind in "iu")
    if as_int:
        if interp != "nearest":
            raise ValueError("an integer volume is resampled with interp='nearest'")
        t = vol if is_t else torch.from_numpy(np.ascontiguousarray(vol).astype(np.int32))
        src = t.to(dev, torch.int32).contiguous()
    else:
        src = _f32_dev(vol, dev)
    oz, oy, ox = dst_geom.shape
    out = torch.empty((n_vol, oz, oy, ox) if len(shape) == 4 else (oz, oy, ox), dtype=src.dtype, device=dev)
    with torch.cuda.device(dev):
        check(lib.t2fit_resample_dev(src.data_ptr(), _abi.RESAMPLE_I32 if as_int else _abi.RESAMPLE_F32, *shape[-3:],
                                     A.ctypes.data_as(C.POINTER(C.c_double)), out.data_ptr(), oz, oy, ox, n_vol,
                                     _abi.INTERPS[interp], float(default), _abi.RESAMPLE_INTEGER_CAST if integer_cast else 0,
                                     _current_stream()))
        src.record_stream(torch.cuda.current_stream())
    return (out if is_t else out.cpu().numpy()), dst_geom


RECON_FORMS = ("chain", "fused")


def reconstruct_stacks(stacks, geoms, *, fixed="ax", res=1.0, transforms=None, integer_cast=False, form="chain", device=0):
    """Steps 1 and 2 of the reference's run_qmri_reconstruction.py on the GPU, registration excepted: ``stacks`` =
    {"ax", "cor", "sag": float32 ``(nTE, Z, Y, X)`` (or ``(Z, Y, X)``) thick-slice stack, numpy or CUDA tensor}, ``geoms``
    their geometries (``nifti.Image`` or anything with GetSpacing / GetOrigin / GetDirection).  Every stack is resampled to
    ``res`` mm isotropic, the two moving ones onto the ``fixed`` one's grid through ``transforms`` ({orientation: 4 x 4,
    fixed point -> moving point}; identity where absent), and the three are averaged.  ``form``: ``'chain'`` (single-stage
    passes and a merge, with a workspace: the faster one at 256^3 x 8, hence the default) or ``'fused'`` (one kernel, no
    intermediate volume, no workspace); same bits.
    Returns ``(echoes, header)``: a float32 CUDA tensor ``(nTE, Z, Y, X)`` on the fixed grid -- what :func:`denoise_tv` and
    :func:`fit_volume` take -- asynchronous on the current stream, and a ``nifti.Image`` over an empty array that carries
    the grid's spacing, origin and direction.  Fewer than three orientations: ValueError (the reference skips such an
    echo).  :func:`fetal_t2mapping_amd._resample.reconstruct` states the definition in numpy."""
    import torch

    from . import _resample

    lib = _require(*_RECON_SYMBOLS)
    if form not in RECON_FORMS:
        raise ValueError(f"form must be one of {RECON_FORMS}, got {form!r}")
    missing = [o for o in _resample.ORIENTATIONS if o not in stacks or o not in geoms]
    if missing:
        raise ValueError(f"the reconstruction needs the three orientations ax, cor, sag; missing: {', '.join(missing)}")
    shapes = {o: tuple(int(v) for v in stacks[o].shape) for o in _resample.ORIENTATIONS}
    if any(len(s) not in (3, 4) for s in shapes.values()) or len({len(s) for s in shapes.values()}) != 1:
        raise ValueError(f"the stacks must all be (Z, Y, X) or all (nTE, Z, Y, X), got {shapes}")
    n_vols = {s[0] if len(s) == 4 else 1 for s in shapes.values()}
    if len(n_vols) != 1:
        raise ValueError(f"the stacks differ in their number of echoes: {shapes}")
    n_vol = n_vols.pop()
    order, hi, a1, a2 = _resample.plan({o: _resample.as_geometry(geoms[o], shapes[o][-3:]) for o in _resample.ORIENTATIONS},
                                       fixed, res, transforms)
    dev = _roi_device([stacks[o] for o in order], device)
    src = [_f32_dev(stacks[o], dev) for o in order]
    lo_size = (C.c_int32 * 9)(*[v for o in order for v in shapes[o][-3:]])
    hi_size = (C.c_int32 * 9)(*[v for g in hi for v in g.shape])
    A1 = (C.c_double * 36)(*np.concatenate([a.ravel() for a in a1]))
    A2 = (C.c_double * 24)(*np.concatenate([a.ravel() for a in a2]))
    flags = (_abi.RESAMPLE_INTEGER_CAST if integer_cast else 0) | (_abi.RECON_CHAIN if form == "chain" else 0)
    need = C.c_size_t(0)
    check(lib.t2fit_reconstruct_workspace_bytes(n_vol, lo_size, hi_size, flags, C.byref(need)))
    out = torch.empty((n_vol,) + hi[0].shape, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws, ws_ptr = _workspace(need.value, dev) if need.value else (None, None)
        ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in src])
        check(lib.t2fit_reconstruct_dev(ptrs, lo_size, A1, hi_size, A2, out.data_ptr(), n_vol, flags, ws_ptr, need.value,
                                        _current_stream()))
        for t in src + ([ws] if ws is not None else []):
            t.record_stream(torch.cuda.current_stream())
    return out, _geometry_header(hi[0])


# --------------------------------------------------------------------------------------------
# masks and phantom labels: binary morphology, hole filling, seed labels (utils/qmri_utils.py build_mask :223-252,
# build_phantom_masks :591-623, build_phantom_labels_v2 :868-933, build_mask_from_labels :935-951,
# convert_synthseg_to_feta :976-1009)
# --------------------------------------------------------------------------------------------
_MORPH_SYMBOLS = _abi.ADDITIVE[9:15]


def _volume_dev(a, dtype, device, what="volume"):
    """A 3-D numpy array or tensor -> contiguous tensor of `dtype` on the GPU (a mask: 0 / not 0 -> uint8 0 / 1)."""
    import torch

    t = a if _is_tensor(a) else torch.from_numpy(np.ascontiguousarray(a))
    if t.dim() != 3:
        raise ValueError(f"{what} must be 3-D (z, y, x), got shape {tuple(t.shape)}")
    dev = t.device if t.is_cuda else torch.device("cuda", device)
    if dtype == torch.uint8 and t.dtype != torch.uint8:
        t = t != 0
    return t.to(dev, dtype).contiguous()


def _element(element):
    """(runs int32 (n, 4), size int32 (3,)) from a boolean footprint or a ``(runs, size)`` pair."""
    from . import _morph

    runs, size = _morph._as_runs(element)
    _morph._footprint(np.zeros(size, bool))  # odd sizes, radius <= 32: the message names the footprint
    return np.ascontiguousarray(runs, np.int32), np.asarray(size, np.int32)


def _morph_workspace(lib, shape, reach, dev):
    need = C.c_size_t(0)
    check(lib.t2fit_morph_workspace_bytes(shape[0], shape[1], shape[2], int(reach), C.byref(need)))
    ws, ptr = _workspace(need.value, dev)
    return ws, ptr, need.value


def binary_threshold(vol, lo=-np.inf, hi=np.inf, *, device=0):
    """``lo <= vol <= hi`` as a uint8 (0 / 1) CUDA tensor shaped like ``vol``: a float32 or int32 numpy array or tensor
    (other dtypes are converted to float32, integer ones to int32).  The comparison is exact; a NaN gives 0."""
    import torch

    lib = _require(*_MORPH_SYMBOLS)
    t = vol if _is_tensor(vol) else torch.from_numpy(np.ascontiguousarray(vol))
    integer = not t.dtype.is_floating_point
    dev = t.device if t.is_cuda else torch.device("cuda", device)
    t = t.to(dev, torch.int32 if integer else torch.float32).contiguous()
    out = torch.empty(t.shape, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.t2fit_binary_threshold_dev(t.data_ptr(), _abi.MORPH_I32 if integer else _abi.MORPH_F32, t.numel(), float(lo),
                                             float(hi), out.data_ptr(), _current_stream()))
    return out


def _binary_morph(op, mask, element, iterations, border_value, unbounded, out, device):
    import torch

    lib = _require(*_MORPH_SYMBOLS)
    runs, size = _element(element)
    m = _volume_dev(mask, torch.uint8, device, "mask")
    if out is None:
        out = torch.empty_like(m)
    elif not (_is_tensor(out) and out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
              and out.shape == m.shape and out.device == m.device):
        raise ValueError("out must be a contiguous uint8 CUDA tensor of the mask's shape on the mask's device")
    reach = int(size.max() // 2) * int(iterations) if unbounded else 0
    with torch.cuda.device(m.device):
        ws, ptr, nbytes = _morph_workspace(lib, m.shape, reach, m.device)
        check(lib.t2fit_binary_morph_dev(_abi.MORPH_OPS[op], m.data_ptr(), out.data_ptr(), m.shape[0], m.shape[1], m.shape[2],
                                         size.ctypes.data, runs.ctypes.data, len(runs), int(iterations), int(border_value),
                                         _abi.MORPH_UNBOUNDED if unbounded else 0, ptr, nbytes, _current_stream()))
        ws.record_stream(torch.cuda.current_stream())
    return out


def binary_dilate(mask, element, *, iterations=1, border_value=0, out=None, device=0):
    """``scipy.ndimage.binary_dilation(mask, element, iterations, border_value=...)`` on the GPU.  ``mask``: 3-D numpy
    array or tensor (0 / not 0); ``element``: a boolean footprint with odd sizes up to 65 (``_morph.ball`` / ``box`` /
    ``cross`` or any other) or its ``(runs, size)`` pair.  Returns a uint8 CUDA tensor; ``out`` may be the input."""
    return _binary_morph("dilate", mask, element, iterations, border_value, False, out, device)


def binary_erode(mask, element, *, iterations=1, border_value=0, out=None, device=0):
    """``scipy.ndimage.binary_erosion``: the exact dual of :func:`binary_dilate`."""
    return _binary_morph("erode", mask, element, iterations, border_value, False, out, device)


def binary_close(mask, element, *, iterations=1, border_value=0, unbounded=False, out=None, device=0):
    """Dilations, then erosions.  ``unbounded=False``: scipy's ``binary_closing`` (each half sees ``border_value``
    outside).  ``unbounded=True``: the closing on the unbounded domain -- pad with zeros by the element's reach, close,
    crop -- which keeps an object near the border from being eaten by the erosion (ITK's safe border)."""
    return _binary_morph("close", mask, element, iterations, border_value, unbounded, out, device)


def binary_open(mask, element, *, iterations=1, border_value=0, unbounded=False, out=None, device=0):
    """Erosions, then dilations; the two forms as in :func:`binary_close`."""
    return _binary_morph("open", mask, element, iterations, border_value, unbounded, out, device)


def fill_holes(mask, *, slice_axis=None, out=None, return_sweeps=False, device=0):
    """``scipy.ndimage.binary_fill_holes`` on the GPU (face connectivity).  ``slice_axis`` in (0, 1, 2): every plane
    perpendicular to that axis of the (z, y, x) array is filled on its own.  Returns a uint8 CUDA tensor (and the number
    of tile sweeps with ``return_sweeps``).  The call waits for the current stream: the host watches the flood end."""
    import torch

    lib = _require(*_MORPH_SYMBOLS)
    if slice_axis not in (None, 0, 1, 2):
        raise ValueError("slice_axis must be None, 0, 1 or 2")
    m = _volume_dev(mask, torch.uint8, device, "mask")
    if out is None:
        out = torch.empty_like(m)
    sweeps = C.c_int32(0)
    with torch.cuda.device(m.device):
        ws, ptr, nbytes = _morph_workspace(lib, m.shape, 0, m.device)
        check(lib.t2fit_fill_holes_dev(m.data_ptr(), out.data_ptr(), m.shape[0], m.shape[1], m.shape[2],
                                       -1 if slice_axis is None else int(slice_axis), ptr, nbytes, C.byref(sweeps),
                                       _current_stream()))
        ws.record_stream(torch.cuda.current_stream())
    return (out, int(sweeps.value)) if return_sweeps else out


def seed_labels(shape, seeds, element, *, labels=None, dtype="uint8", device=0):
    """``out[v] = max over seeds s of labels[s] * [v - seed_s in element]`` as a CUDA tensor of ``shape`` (z, y, x).
    ``seeds``: ``(x, y, z)`` indices, as the reference indexes an image; ``labels`` default to 1..n; ``dtype``
    'uint8' or 'int32'.  What leaves the volume is clipped."""
    import torch

    lib = _require(*_MORPH_SYMBOLS)
    runs, size = _element(element)
    sd = np.ascontiguousarray(np.asarray(seeds, np.int64).reshape(-1, 3), np.int32)
    lab = np.ascontiguousarray(np.arange(1, len(sd) + 1) if labels is None else labels, np.int32)
    if lab.shape != (len(sd),):
        raise ValueError("labels must have one entry per seed")
    if dtype not in ("uint8", "int32"):
        raise ValueError("dtype must be 'uint8' or 'int32'")
    shape = tuple(int(v) for v in shape)
    if len(shape) != 3:
        raise ValueError(f"shape must be (z, y, x), got {shape}")
    dev = torch.device("cuda", device)
    out = torch.empty(shape, dtype=torch.uint8 if dtype == "uint8" else torch.int32, device=dev)
    with torch.cuda.device(dev):
        ws, ptr, nbytes = _morph_workspace(lib, shape, 0, dev)
        check(lib.t2fit_seed_labels_dev(sd.ctypes.data, lab.ctypes.data, len(sd), size.ctypes.data, runs.ctypes.data, len(runs),
                                        shape[0], shape[1], shape[2], out.data_ptr(),
                                        _abi.MORPH_U8 if dtype == "uint8" else _abi.MORPH_I32, ptr, nbytes, _current_stream()))
        ws.record_stream(torch.cuda.current_stream())
    return out


def relabel(labels, lut, *, device=0):
    """``lut[labels]`` where ``0 <= labels < len(lut)``, else 0: an int32 CUDA tensor shaped like ``labels``."""
    import torch

    lib = _require(*_MORPH_SYMBOLS)
    lab = _int_tensor(labels)
    dev = lab.device if lab.is_cuda else torch.device("cuda", device)
    lab = lab.to(dev)
    if lab.dtype != torch.int32:  # ids beyond int32 are outside every table
        lab = torch.where((lab >= 0) & (lab < 2**31), lab, torch.full_like(lab, -1)).to(torch.int32)
    lab = lab.contiguous()
    table = torch.from_numpy(np.ascontiguousarray(lut, np.int32)).to(dev)
    out = torch.empty_like(lab)
    with torch.cuda.device(dev):
        check(lib.t2fit_relabel_dev(lab.data_ptr(), lab.numel(), table.data_ptr(), table.numel(), out.data_ptr(),
                                    _current_stream()))
        table.record_stream(torch.cuda.current_stream())
    return out


def _above(threshold):
    """The smallest float32 strictly above `threshold`: ``v > threshold`` for a float32 v is ``v >= _above(threshold)``."""
    f = np.float32(threshold)
    return float(f) if float(f) > float(threshold) else float(np.nextafter(f, np.float32(np.inf)))


def build_mask(vol, threshold=1.0, slice_axis=2, size=5, *, device=0):
    """The reference's ``build_mask``: ``vol > threshold``, then per plane perpendicular to ``slice_axis`` of the
    (z, y, x) array: fill holes, dilate and erode with a ``size x size`` square (scipy's borders).  uint8 CUDA tensor."""
    if size < 1 or size % 2 == 0:
        raise ValueError("size must be odd")
    fp_shape = [size, size, size]
    fp_shape[slice_axis] = 1
    square = np.ones(fp_shape, bool)
    m = binary_threshold(np.asarray(vol, np.float32) if not _is_tensor(vol) else vol.float(), _above(threshold), device=device)
    m = fill_holes(m, slice_axis=slice_axis, out=m)
    m = binary_dilate(m, square, out=m)
    return binary_erode(m, square, out=m)


def phantom_mask(vol, threshold=100, close_radius=15, dilate_radius=10, *, device=0):
    """The reference's ``build_phantom_masks`` for one echo volume: ``vol >= threshold``, 3-D fill holes, closing with
    the radius-``close_radius`` ball on the unbounded domain, dilation with the radius-``dilate_radius`` ball
    (:func:`_morph.ball`).  uint8 CUDA tensor."""
    from . import _morph

    m = binary_threshold(np.asarray(vol, np.float32) if not _is_tensor(vol) else vol.float(), float(threshold), device=device)
    m = fill_holes(m, out=m)
    m = binary_close(m, _morph.ball(close_radius), unbounded=True, out=m)
    return binary_dilate(m, _morph.ball(dilate_radius), out=m)


def phantom_labels(shape, seeds, radius=6, *, device=0):
    """The reference's ``build_phantom_labels_v2``: a radius-``radius`` ball at every ``(x, y, z)`` seed carrying the
    seed's 1-based number, merged with a maximum.  uint8 CUDA tensor of ``shape`` (z, y, x)."""
    from . import _morph

    return seed_labels(shape, seeds, _morph.ball(radius), device=device)


def mask_from_labels(labels, *, device=0):
    """The reference's ``build_mask_from_labels``: ``labels >= 1`` as a uint8 CUDA tensor."""
    import torch

    lab = _int_tensor(labels)
    dev = lab.device if lab.is_cuda else torch.device("cuda", device)
    lab = lab.to(dev).clamp(min=-1, max=1).to(torch.int32)  # the sign is all that matters; int64 ids stay in range
    return binary_threshold(lab, 1, device=device)


def synthseg_to_feta(labels, *, device=0):
    """The reference's ``convert_synthseg_to_feta``: SynthSeg ids -> FeTA tissue classes 1..7, everything else 0
    (``_morph.SYNTHSEG_TO_FETA``).  int32 CUDA tensor."""
    from . import _morph

    return relabel(labels, _morph.feta_lut(), device=device)


def _boot_config(TEeffs):
    """The synthesis reads n_te and te_ms of a config and nothing else."""
    return make_config("gaussian", fit_table("gaussian", True), TEeffs)


def synth_replica(t2, k, TEeffs, noise_sigma, mask, *, seed, replica, noise="rician", voxel_offset=0, device=0):
    """Replica ``replica`` of the acquisition under ``seed``: ``sqrt((S + s n1)**2 + (s n2)**2)`` (``noise='rician'``) or
    ``S + s n1`` (``'gaussian'``) with ``S = k exp(-TE / T2)`` and the counter-based normal pairs of
    :mod:`fetal_t2mapping_amd._philox`, made on the GPU.  ``t2`` / ``k``: ``(Z, Y, X)`` float32 maps (numpy or CUDA
    tensor), ``noise_sigma``: a number or a map of that shape, ``mask``: that shape or None.  Returns a float32 CUDA tensor
    ``(nTE, Z, Y, X)`` that :func:`fit_volume` takes as it stands; voxels outside the mask are 0.  A sample depends on
    (seed, flat voxel index, echo, replica) alone; ``voxel_offset`` is the flat index of this block's first voxel in the
    volume the stream refers to (a slab ``[z0:z1]`` with ``voxel_offset = z0 * Y * X`` equals those rows of the whole)."""
    import torch

    lib = _require(*_BOOT_SYMBOLS)
    cfg = _boot_config(TEeffs)
    spatial = tuple(t2.shape)
    n = int(np.prod(spatial)) if len(spatial) else 1
    dev = _roi_device((t2, k, mask), device)
    t2_d, k_d = _f32_dev(t2, dev), _f32_dev(k, dev, n, "k")
    m = None if mask is None else _mask_dev(mask, dev, n)
    scalar, s_d = (float(noise_sigma), None) if np.ndim(noise_sigma) == 0 else (0.0, _f32_dev(noise_sigma, dev, n, "noise_sigma"))
    out = torch.empty((cfg.n_te,) + spatial, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.t2fit_boot_synth_dev(C.byref(cfg), t2_d.data_ptr(), k_d.data_ptr(), scalar,
                                       None if s_d is None else s_d.data_ptr(), None if m is None else m.data_ptr(), n,
                                       int(voxel_offset), int(seed) & (2 ** 64 - 1), int(replica), _noise_kind(noise),
                                       out.data_ptr(), _current_stream()))
    return out


def bootstrap_volume(echoes, mask, TEeffs, fit, fit_params, prior=True, *, n_replicas=100, seed=0, alpha=0.05,
                     noise_sigma="background", noise="rician", params=("t2",), interval=True, layout="te_major",
                     solver="lbfgsb", precision="f64", maps: T2Maps = None, numpy_legacy=False, device=0) -> BootMaps:
    """Parametric bootstrap of the fit as it is run: simulate the acquisition from the fitted (k, T2) with noise of level
    ``noise_sigma``, refit with the same solver, bounds, prior and stop rules, ``n_replicas`` times, and reduce every
    voxel's refits to bias, standard deviation and a percentile interval -- all on the GPU, inside the library
    (t2fit_bootstrap_dev: replica r + 1 is synthesised while replica r is fitted).

    ``echoes`` / ``mask`` / ``TEeffs`` / ``fit`` / ``fit_params`` / ``prior`` / ``solver`` / ``precision`` as in
    :func:`fit_volume` (numpy arrays or CUDA tensors); the volume is fitted first unless ``maps`` (a :class:`T2Maps` of
    it) is given -- then ``echoes`` is only read for ``noise_sigma='background'`` and may be None otherwise.
    ``noise_sigma``: ``'background'`` (:func:`estimate_background_sigma`), ``'sigma_map'`` (the fitted sigma of every
    voxel; not for ``'gaussian'``, which has none), a number, or a map.  ``params``: any of ``'t2'``, ``'k'``,
    ``'sigma'``.  ``interval=False`` leaves the percentiles out (no limit on ``n_replicas`` then; with them at most
    512).  Returns :class:`BootMaps` of numpy arrays for numpy input, of CUDA tensors for tensor input; the results
    depend on the arguments alone.  Normalised fits (``norm``) are not supported."""
    import torch

    lib = _require(*_BOOT_SYMBOLS)
    cfg = make_config(fit, fit_params, TEeffs, prior, False, solver, precision, numpy_legacy)
    params = tuple(params)
    if not params or any(p not in _abi.BOOT_PARAMS for p in params):
        raise ValueError(f"params must be a non-empty subset of {tuple(_abi.BOOT_PARAMS)}, got {params!r}")
    if fit == "gaussian" and "sigma" in params:
        raise ValueError("the 2-parameter 'gaussian' fit has no sigma to bootstrap")
    # what noise_sigma is, decided once: a map must never be compared with a string (numpy compares elementwise)
    from_background = isinstance(noise_sigma, str) and noise_sigma == "background"
    from_sigma_map = isinstance(noise_sigma, str) and noise_sigma == "sigma_map"
    if isinstance(noise_sigma, str) and not (from_background or from_sigma_map):
        raise ValueError("noise_sigma must be 'background', 'sigma_map', a number or a map")
    if from_sigma_map and fit == "gaussian":
        raise ValueError("noise_sigma='sigma_map' needs a fitted sigma: the 2-parameter 'gaussian' fit has none")
    kind = _noise_kind(noise)
    n_replicas = int(n_replicas)
    if interval and not 2 <= n_replicas <= _abi.BOOT_MAX_INTERVAL_REPLICAS:
        raise ValueError(f"a percentile interval needs 2..{_abi.BOOT_MAX_INTERVAL_REPLICAS} replicas (got {n_replicas}); "
                         "interval=False computes the moments for any number")
    if interval and not 0.0 < float(alpha) < 1.0:
        raise ValueError("alpha must lie in (0, 1)")
    if echoes is None and (maps is None or from_background):
        raise ValueError("echoes is needed to fit the volume and for noise_sigma='background'")
    given = [a for a in (echoes, maps.t2 if maps is not None else None) if a is not None]
    as_torch = _is_tensor(given[0])
    dev = _roi_device(given + [mask], device)
    e_t = echoes  # (uploaded once: the fit and the background level read the same device copy)
    if maps is None:
        e_t = echoes if as_torch else torch.from_numpy(np.ascontiguousarray(echoes, dtype=np.float32)).to(dev)
        lay, spatial = _layout_of(e_t.shape, cfg.n_te, layout)
        m = _mask_dev(mask, dev, int(np.prod(spatial)))
        maps_d = fit_volume(e_t, m, TEeffs, fit, fit_params, prior=prior, layout=layout, solver=solver, precision=precision,
                            extras=True, numpy_legacy=numpy_legacy)
    else:
        spatial = tuple(maps.t2.shape)
        m = _mask_dev(mask, dev, int(np.prod(spatial)))
        maps_d = maps
    n = int(np.prod(spatial)) if len(spatial) else 1
    t2_d, k_d = _f32_dev(maps_d.t2, dev, n, "maps.t2"), _f32_dev(maps_d.k, dev, n, "maps.k")
    sg_d = _f32_dev(maps_d.sigma, dev, n, "maps.sigma") if ("sigma" in params or from_sigma_map) else None
    scalar, s_d = 0.0, None
    if from_background:
        scalar, _ = estimate_background_sigma(e_t, m.reshape(spatial), layout=layout, device=dev.index or 0)
    elif from_sigma_map:
        s_d = sg_d
    elif np.ndim(noise_sigma) == 0:
        scalar = float(noise_sigma)
    else:
        s_d = _f32_dev(noise_sigma, dev, n, "noise_sigma")
    out = _abi.T2FitBootMaps()
    stats = {}
    for p in params:
        i = _abi.BOOT_PARAMS[p]
        new = lambda: torch.empty(spatial, dtype=torch.float32, device=dev)  # noqa: E731
        stats[p] = BootStats(new(), new(), new(), new() if interval else None, new() if interval else None)
        for name in ("mean", "bias", "std", "ci_lo", "ci_hi"):
            t = getattr(stats[p], name)
            getattr(out, name)[i] = None if t is None else t.data_ptr()
    n_ok = torch.empty(spatial, dtype=torch.int32, device=dev)
    out.n_ok = n_ok.data_ptr()
    which = sum(1 << _abi.BOOT_PARAMS[p] for p in set(params))
    with torch.cuda.device(dev):
        check(lib.t2fit_bootstrap_dev(None, C.byref(cfg), t2_d.data_ptr(), k_d.data_ptr(),
                                      None if sg_d is None else sg_d.data_ptr(), scalar, None if s_d is None else s_d.data_ptr(),
                                      kind, m.data_ptr(), n, n_replicas, int(seed) & (2 ** 64 - 1), float(alpha), which,
                                      C.byref(out), 0,
                                      _current_stream()))
    host = (lambda t: t) if as_torch else (lambda t: None if t is None else t.cpu().numpy())
    if not as_torch:
        for p in stats:
            stats[p] = BootStats(*(host(getattr(stats[p], name)) for name in ("mean", "bias", "std", "ci_lo", "ci_hi")))
        if maps is None:
            maps_d = T2Maps(*(host(getattr(maps_d, name)) for name in ("t2", "k", "sigma", "res", "r2", "fun", "nit", "status", "t2_se")))
    return BootMaps(stats.get("t2"), stats.get("k"), stats.get("sigma"), host(n_ok), maps_d,
                    None if s_d is not None else float(scalar), n_replicas, int(seed), float(alpha))
