"""Multi-component T2 spectra on the GPU (``t2map.spectrum``): a non-negative T2 distribution per voxel by regularised
non-negative least squares, a wave per voxel, at one weight for the volume (``solve``) or at a weight chosen per voxel by the
chi^2 rule (``solve_chi2``); :mod:`fetal_t2mapping_amd._nnls` states the result in numpy and holds the builders both paths share."""
import ctypes as C

import numpy as np

from . import _abi
from ._gpu import current_stream, flat, is_tensor, mask_u8, pick_device, release, require
from ._gpu_fit import T2Maps
from ._lib import check, load
from ._nnls import (Basis, derived, ln_t2_functional, log_grid, monoexp_basis, window_functionals)  # noqa: F401  (the namespace's builders)

DEFAULT_MU = 0.03  # chosen on the CPU statement from one sweep on synth.py's phantom (README, "T2 spectra")


def params(tol_rel=None, piv_rel=None, max_iter=None, max_blocks=None):
    """The library's defaults with the given fields replaced."""
    p = _abi.T2FitNnlsParams()
    check(load().t2fit_nnls_params_default(C.byref(p)))
    for name, value in (("tol_rel", tol_rel), ("piv_rel", piv_rel), ("max_iter", max_iter), ("max_blocks", max_blocks)):
        if value is not None:
            setattr(p, name, value)
    return p


def chi2_params(factor=None, mu_first=None, grow=None, n_grow=None, n_bisect=None, exact_rel=None, mu_exact=None):
    """The library's numbers of the chi^2 rule (factor 1.02, first weight 1e-3, growth 4 over 6 steps, 5 bisections; an exact
    fit -- misfit at most 1e-12 of sum y^2 -- gets ``DEFAULT_MU``) with the given fields replaced."""
    p = _abi.T2FitNnlsChi2Params()
    check(load().t2fit_nnls_chi2_params_default(C.byref(p)))
    for name, value in (("factor", factor), ("mu_first", mu_first), ("grow", grow), ("n_grow", n_grow), ("n_bisect", n_bisect),
                        ("exact_rel", exact_rel), ("mu_exact", mu_exact)):
        if value is not None:
            setattr(p, name, value)
    return p


def workgroup(n_basis):
    """``(waves, lds_bytes, workgroups_per_cu)``: the launch shape the library uses for this basis size, asked of the library
    (``t2fit_nnls_workgroup``; no device).  Each wave has one voxel in flight and takes ``_abi.NNLS_CHUNK`` voxels at a time."""
    waves, lds, per_cu = C.c_int(0), C.c_size_t(0), C.c_int(0)
    check(load().t2fit_nnls_workgroup(int(n_basis), C.byref(waves), C.byref(lds), C.byref(per_cu)))
    return waves.value, lds.value, per_cu.value


def workgroup_waves(n_basis):
    """Waves of the kernel's workgroup for this basis size."""
    return workgroup(n_basis)[0]


def pack(basis):
    """The packed basis (``uint8`` numpy array) as ``t2fit_nnls_pack_host`` writes it; no device."""
    a = np.ascontiguousarray(basis.A, dtype=np.float64)
    w = np.ascontiguousarray(basis.W, dtype=np.float64)
    lib = load()
    need = C.c_size_t(0)
    check(lib.t2fit_nnls_pack_bytes(a.shape[0], a.shape[1], w.shape[0], C.byref(need)))
    out = np.zeros(need.value, np.uint8)
    check(lib.t2fit_nnls_pack_host(a.shape[0], a.shape[1], w.shape[0], a.ctypes.data, float(basis.mu), w.ctypes.data if w.shape[0] else None,
                                   out.ctypes.data, out.nbytes))
    return out


def _packed_on(basis, dev):
    """The packed block on `dev`; the :class:`Basis` keeps it for the next call."""
    import torch

    cache = getattr(basis, "_packed_dev", None)
    key = str(dev)
    if cache is not None and key in cache:
        return cache[key]
    t = torch.from_numpy(pack(basis)).to(dev)
    if t.data_ptr() % 16:
        raise RuntimeError("the device allocator returned a block that is not aligned to 16 bytes")
    if cache is None:
        cache = basis._packed_dev = {}
    cache[key] = t
    return t


def _basis_for(basis, mu, functionals):
    """`basis` with `mu` and `functionals` (``(W, names)``) replaced where given; the same object when nothing changes, so
    that its packed block is reused."""
    if mu is None and functionals is None:
        return basis
    W, names = (basis.W, basis.names) if functionals is None else functionals
    mu = basis.mu if mu is None else float(mu)
    W = np.asarray(W, np.float64).reshape(-1, basis.n_basis)
    if mu == basis.mu and tuple(names) == basis.names and np.array_equal(W, basis.W):
        return basis
    return Basis(basis.A, mu, W, names, basis.t2_grid)


def _solve(echoes, basis, mask, spectrum, device, solver_params, chi2):
    """Both entry points: ``chi2`` None calls ``t2fit_nnls_dev``, a ``T2FitNnlsChi2Params`` calls ``t2fit_nnls_chi2_dev`` and adds its
    four outputs."""
    import torch

    lib = require(*(_abi.NNLS_SYMBOLS + (_abi.NNLS_CHI2_SYMBOLS if chi2 is not None else ())))
    shape = tuple(int(v) for v in echoes.shape)
    if len(shape) < 1 or shape[0] != basis.n_te:
        raise ValueError(f"the echoes are TE-major with {shape[0] if shape else 0} echoes, the basis has {basis.n_te}")
    spatial = shape[1:]
    n_vox = int(np.prod(spatial, dtype=np.int64))
    dev = pick_device((echoes, mask), device)
    p = solver_params if solver_params is not None else params()
    with torch.cuda.device(dev):
        packed = _packed_on(basis, dev)
        y = flat(echoes, dev)
        msk = None if mask is None else mask_u8(mask, dev, n_vox)
        x = torch.empty((basis.n_basis, n_vox), dtype=torch.float32, device=dev) if spectrum else None
        func = torch.empty((basis.n_func, n_vox), dtype=torch.float32, device=dev)
        amp = torch.empty(n_vox, dtype=torch.float32, device=dev)
        rmse = torch.empty(n_vox, dtype=torch.float32, device=dev)
        nit = torch.empty(n_vox, dtype=torch.int32, device=dev)
        status = torch.empty(n_vox, dtype=torch.int32, device=dev)
        common = (y.data_ptr(), basis.n_te, n_vox, None if msk is None else msk.data_ptr(), packed.data_ptr(),
                  None if x is None else x.data_ptr(), func.data_ptr() if basis.n_func else None, amp.data_ptr(), rmse.data_ptr(),
                  nit.data_ptr(), status.data_ptr())
        extra = {}
        if chi2 is None:
            check(lib.t2fit_nnls_dev(C.byref(p), *common, current_stream()))
        else:
            extra = {"mu": torch.empty(n_vox, dtype=torch.float32, device=dev), "ratio": torch.empty(n_vox, dtype=torch.float32, device=dev),
                     "solves": torch.empty(n_vox, dtype=torch.int32, device=dev), "rule": torch.empty(n_vox, dtype=torch.int32, device=dev)}
            check(lib.t2fit_nnls_chi2_dev(C.byref(p), C.byref(chi2), *common, *(t.data_ptr() for t in extra.values()), current_stream()))
        release(y, msk)
    out = {"func": func.reshape((basis.n_func,) + spatial), "amp": amp.reshape(spatial), "rmse": rmse.reshape(spatial),
           "nit": nit.reshape(spatial), "status": status.reshape(spatial)}
    if spectrum:
        out["x"] = x.reshape((basis.n_basis,) + spatial)
    out.update({k: t.reshape(spatial) for k, t in extra.items()})
    return out


def solve(echoes, basis, mask=None, mu=None, functionals=None, spectrum=False, device=0, solver_params=None):
    """A dict of CUDA tensors of the echoes' spatial shape: ``func`` float32 ``(n_func, ...)``, ``amp``, ``rmse`` float32, ``nit``,
    ``status`` int32 and, with ``spectrum=True``, ``x`` float32 ``(n_basis, ...)``.  ``echoes``: float32 ``(nTE, ...)``, numpy array
    or tensor; ``basis``: a :class:`Basis`; ``mu`` and ``functionals`` (``(W, names)``) replace the basis's own when given;
    ``mask``: 0 / not 0 of the spatial shape, or None.  Bit for bit :func:`_nnls.solve`."""
    if not isinstance(basis, Basis):
        raise ValueError("solve takes a Basis (t2map.spectrum.Basis)")
    return _solve(echoes, _basis_for(basis, mu, functionals), mask, spectrum, device, solver_params, None)


def _basis_mu0(basis, functionals=None):
    """`basis` at weight 0 for the rule; the repacked one is kept on `basis`, so that its packed block is reused."""
    if functionals is not None or basis.mu == 0:
        return _basis_for(basis, 0.0, functionals)
    if getattr(basis, "_mu0", None) is None:
        basis._mu0 = basis.with_mu(0.0)
    return basis._mu0


def solve_chi2(echoes, basis, mask=None, functionals=None, spectrum=False, device=0, solver_params=None, chi2=None):
    """:func:`solve` with the weight chosen per voxel by the chi^2 rule (include/t2fit.h): the dict of :func:`solve`, from each
    voxel's final solve with ``nit`` summed and ``status`` the largest over its solves, plus ``mu``, ``ratio`` float32 (the chosen
    weight; its misfit over the unregularised one) and ``solves``, ``rule`` int32 (``_abi.NNLS_RULE_*``, -1 where nothing was
    fitted).  The basis's own ``mu`` is not used: a basis with ``mu != 0`` is repacked at 0.  ``chi2``: :func:`chi2_params`, or
    None for the library's.  Bit for bit :func:`_nnls.solve_chi2`."""
    if not isinstance(basis, Basis):
        raise ValueError("solve_chi2 takes a Basis (t2map.spectrum.Basis)")
    return _solve(echoes, _basis_mu0(basis, functionals), mask, spectrum, device, solver_params, chi2 if chi2 is not None else chi2_params())


def spectrum_basis(te_ms, t2_grid, mu=DEFAULT_MU, windows=None):
    """The :class:`Basis` of a T2 spectrum: ``exp(-TE / T2)`` over the grid, the functional ``lnT2`` (for the geometric mean)
    and one 0 / 1 functional per window ``{name: (lo, hi)}`` [ms]."""
    grid = np.asarray(t2_grid, np.float64).reshape(-1)
    W, names = window_functionals(grid, windows or {})
    if "lnT2" in names:
        raise ValueError("a window cannot be named lnT2")
    return Basis(monoexp_basis(te_ms, grid), mu, np.vstack([ln_t2_functional(grid)[None, :], W]), ("lnT2",) + names, grid)


def fit_volume_nnls(echoes, mask, basis, device=0, spectrum=False, chi2=None):
    """The spectrum fit as a :class:`T2Maps` plus ``extras``: ``t2`` the geometric-mean T2 ``exp(func_lnT2 / amp)``, ``k`` the
    total amplitude, ``sigma`` zero, ``res`` the RMSE, ``status`` converged / not converged (MAXITER, BREAKDOWN) / masked /
    non-finite; ``extras`` maps ``'<name>fraction'`` for every other functional, ``'nnlsiter'``, ``'nnlsstatus'`` and, with
    ``spectrum=True``, ``'t2spectrum'`` ``(n_basis, ...)`` to their maps.  The ratios are formed with torch in float64 and
    rounded to float32; they are 0 where ``amp`` is not above 0.  numpy echoes give numpy maps, a tensor gives tensors.
    ``chi2``: None fits at the basis's own ``mu``; True, or a dict of :func:`chi2_params` arguments, chooses the weight per voxel
    by the chi^2 rule (:func:`solve_chi2`) and adds ``'nnlsmu'``, ``'nnlschi2'`` (the misfit ratio) float32 and ``'nnlsrule'``,
    ``'nnlssolves'`` int32 to the extras; ``'nnlsiter'`` is then the sum over a voxel's solves."""
    import torch

    if not isinstance(basis, Basis) or "lnT2" not in basis.names:
        raise ValueError("fit_volume_nnls takes a Basis with a functional named lnT2 (spectrum_basis builds one)")
    if chi2 is None or chi2 is False:
        out = solve(echoes, basis, mask, spectrum=spectrum, device=device)
    else:
        out = solve_chi2(echoes, basis, mask, spectrum=spectrum, device=device, chi2=chi2_params(**({} if chi2 is True else dict(chi2))))
    amp64 = out["amp"].double()
    ok = amp64 > 0
    safe = torch.where(ok, amp64, torch.ones_like(amp64))
    zero = torch.zeros((), dtype=torch.float64, device=amp64.device)
    extras = {}
    t2 = None
    for m, name in enumerate(basis.names):
        ratio = out["func"][m].double() / safe
        if name == "lnT2":
            t2 = torch.where(ok, torch.exp(ratio), zero).float()
        else:
            extras[name + "fraction"] = torch.where(ok, ratio, zero).float()
    st = out["status"]
    status = torch.full(st.shape, _abi.ST_NOT_CONV, dtype=torch.uint8, device=st.device)
    status[st == _abi.NNLS_OK] = _abi.ST_CONVERGED
    status[st == _abi.NNLS_MASKED] = _abi.ST_MASKED
    status[st == _abi.NNLS_NONFINITE] = _abi.ST_NONFINITE
    extras["nnlsiter"], extras["nnlsstatus"] = out["nit"], st
    if spectrum:
        extras["t2spectrum"] = out["x"]
    if "rule" in out:
        extras["nnlsmu"], extras["nnlschi2"], extras["nnlsrule"], extras["nnlssolves"] = out["mu"], out["ratio"], out["rule"], out["solves"]
    host = (lambda t: t) if is_tensor(echoes) else (lambda t: t.cpu().numpy())
    maps = T2Maps(t2=host(t2), k=host(out["amp"]), sigma=host(torch.zeros_like(out["amp"])), res=host(out["rmse"]), status=host(status))
    return maps, {n: host(t) for n, t in extras.items()}
