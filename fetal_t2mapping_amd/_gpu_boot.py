"""Parametric bootstrap on the GPU (no reference counterpart): how far to trust a fitted value.  The replica stream is
stated in numpy by :mod:`fetal_t2mapping_amd._philox`."""
import ctypes as C
from dataclasses import dataclass, fields
from typing import Optional

import numpy as np

from . import _abi
from ._gpu import current_stream, flat, is_tensor, mask_u8, pick_device, require
from ._gpu_fit import T2Maps, _layout_of, fit_table, fit_volume, make_config
from ._lib import check


@dataclass
class BootStats:
    """Bootstrap maps of one parameter, ``(Z, Y, X)`` float32: ``mean`` of the counted replicas, ``bias`` = mean - the
    fitted value, ``std`` (ddof = 1, NaN when fewer than two replicas count), ``ci_lo`` / ``ci_hi`` = numpy's default
    percentiles at 100 alpha / 2 and 100 (1 - alpha / 2) (None when no interval was asked for).  Zeros outside the mask.
    Where the fitted value is not finite (``maps=`` with T2 = +inf), ``mean``, ``std`` and the percentiles are still those
    of the counted refits; only ``bias`` is then -inf or NaN."""
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

    lib = require(*_abi.BOOT_SYMBOLS)
    if mask is None:
        raise ValueError("estimate_background_sigma needs a mask: the noise is measured outside it")
    n_te = int(echoes.shape[0] if layout in ("te_major", _abi.LAYOUT_TE_MAJOR) else echoes.shape[-1])
    lay, _, n = _layout_of(echoes.shape, n_te, layout)
    dev = pick_device((echoes, mask), device)
    e = flat(echoes, dev)
    m = mask_u8(mask, dev, n)
    sigma, count = C.c_double(0.0), C.c_int64(0)
    with torch.cuda.device(dev):
        check(lib.t2fit_boot_background_dev(e.data_ptr(), lay, m.data_ptr(), n_te, n, C.byref(sigma), C.byref(count),
                                            current_stream()))
    return float(sigma.value), int(count.value)


def synth_replica(t2, k, TEeffs, noise_sigma, mask, *, seed, replica, noise="rician", voxel_offset=0, device=0):
    """Replica ``replica`` of the acquisition under ``seed``: ``sqrt((S + s n1)**2 + (s n2)**2)`` (``noise='rician'``) or
    ``S + s n1`` (``'gaussian'``) with ``S = k exp(-TE / T2)`` and the counter-based normal pairs of
    :mod:`fetal_t2mapping_amd._philox`, made on the GPU.  ``t2`` / ``k``: ``(Z, Y, X)`` float32 maps (numpy or CUDA
    tensor), ``noise_sigma``: a number or a map of that shape, ``mask``: that shape or None.  Returns a float32 CUDA tensor
    ``(nTE, Z, Y, X)`` that :func:`fit_volume` takes as it stands; voxels outside the mask are 0.  A sample depends on
    (seed, flat voxel index, echo, replica) alone; ``voxel_offset`` is the flat index of this block's first voxel in the
    volume the stream refers to (a slab ``[z0:z1]`` with ``voxel_offset = z0 * Y * X`` equals those rows of the whole)."""
    import torch

    lib = require(*_abi.BOOT_SYMBOLS)
    cfg = make_config("gaussian", fit_table("gaussian", True), TEeffs)  # the synthesis reads n_te and te_ms, nothing else
    spatial = tuple(t2.shape)
    n = int(np.prod(spatial))
    dev = pick_device((t2, k, mask), device)
    t2_d, k_d = flat(t2, dev), flat(k, dev, n, "k")
    m = None if mask is None else mask_u8(mask, dev, n)
    scalar, s_d = (float(noise_sigma), None) if np.ndim(noise_sigma) == 0 else (0.0, flat(noise_sigma, dev, n, "noise_sigma"))
    out = torch.empty((cfg.n_te,) + spatial, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.t2fit_boot_synth_dev(C.byref(cfg), t2_d.data_ptr(), k_d.data_ptr(), scalar,
                                       None if s_d is None else s_d.data_ptr(), None if m is None else m.data_ptr(), n,
                                       int(voxel_offset), int(seed) & (2 ** 64 - 1), int(replica), _noise_kind(noise),
                                       out.data_ptr(), current_stream()))
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

    lib = require(*_abi.BOOT_SYMBOLS)
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
    as_torch = is_tensor(given[0])
    dev = pick_device(given + [mask], device)
    e_t = echoes  # (uploaded once: the fit and the background level read the same device copy)
    if maps is None:
        e_t = echoes if as_torch else flat(echoes, dev).reshape(np.shape(echoes))
        spatial = _layout_of(e_t.shape, cfg.n_te, layout)[1]
    else:
        spatial = tuple(maps.t2.shape)
    n = int(np.prod(spatial))
    m = mask_u8(mask, dev, n)
    maps_d = maps if maps is not None else fit_volume(e_t, m, TEeffs, fit, fit_params, prior=prior, layout=layout, solver=solver,
                                                      precision=precision, extras=True, numpy_legacy=numpy_legacy)
    t2_d, k_d = flat(maps_d.t2, dev, n, "maps.t2"), flat(maps_d.k, dev, n, "maps.k")
    sg_d = flat(maps_d.sigma, dev, n, "maps.sigma") if ("sigma" in params or from_sigma_map) else None
    scalar, s_d = 0.0, None
    if from_background:
        scalar, _ = estimate_background_sigma(e_t, m.reshape(spatial), layout=layout, device=dev.index or 0)
    elif from_sigma_map:
        s_d = sg_d
    elif np.ndim(noise_sigma) == 0:
        scalar = float(noise_sigma)
    else:
        s_d = flat(noise_sigma, dev, n, "noise_sigma")
    out = _abi.T2FitBootMaps()
    stats = {}
    for p in params:
        i = _abi.BOOT_PARAMS[p]
        new = lambda: torch.empty(spatial, dtype=torch.float32, device=dev)  # noqa: E731
        stats[p] = BootStats(new(), new(), new(), new() if interval else None, new() if interval else None)
        for f in fields(BootStats):
            t = getattr(stats[p], f.name)
            getattr(out, f.name)[i] = None if t is None else t.data_ptr()
    n_ok = torch.empty(spatial, dtype=torch.int32, device=dev)
    out.n_ok = n_ok.data_ptr()
    which = sum(1 << _abi.BOOT_PARAMS[p] for p in set(params))
    with torch.cuda.device(dev):
        check(lib.t2fit_bootstrap_dev(None, C.byref(cfg), t2_d.data_ptr(), k_d.data_ptr(),
                                      None if sg_d is None else sg_d.data_ptr(), scalar, None if s_d is None else s_d.data_ptr(),
                                      kind, m.data_ptr(), n, n_replicas, int(seed) & (2 ** 64 - 1), float(alpha), which,
                                      C.byref(out), 0, current_stream()))
    host = (lambda t: t) if as_torch else (lambda t: None if t is None else t.cpu().numpy())
    if not as_torch:
        for p in stats:
            stats[p] = BootStats(*(host(getattr(stats[p], f.name)) for f in fields(BootStats)))
        if maps is None:
            maps_d = T2Maps(*(host(getattr(maps_d, f.name)) for f in fields(T2Maps)))
    return BootMaps(stats.get("t2"), stats.get("k"), stats.get("sigma"), host(n_ok), maps_d,
                    None if s_d is not None else float(scalar), n_replicas, int(seed), float(alpha))
