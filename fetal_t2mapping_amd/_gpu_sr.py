"""Super-resolution reconstruction of the thick-slice stacks on the GPU: the acquisition operator, its adjoint and the
proximal-gradient loop over them; :mod:`fetal_t2mapping_amd._sr` states all three in numpy."""
import ctypes as C

import numpy as np

from . import _abi, _resample, _sr, _svr
from ._gpu import current_stream, flat, is_tensor, pick_device, release, require, workspace
from ._gpu_resample import reconstruct_stacks, resample_volume
from ._gpu_tv import tv_params
from ._lib import check


def _doubles(a):
    a = np.ascontiguousarray(a, np.float64).ravel()
    return (C.c_double * a.size)(*a)


def sr_box(B, profile="box", rel_thickness=1.0):
    """``(Binv (3, 4), radius (x, y, z))`` of t2fit_sr_plan_host for the support of this profile: host arithmetic."""
    lib = require(*_abi.SR_SYMBOLS)
    _, hw = _sr.profile_params(profile, rel_thickness)
    binv, radius = (C.c_double * 12)(), (C.c_int32 * 3)()
    check(lib.t2fit_sr_plan_host(_doubles(np.asarray(B, np.float64).reshape(12)), _doubles((1.0, 1.0, hw)), binv, radius))
    return np.array(binv, np.float64).reshape(3, 4), tuple(int(v) for v in radius)


def _shape4(a, what):
    shape = tuple(int(v) for v in a.shape)
    if len(shape) not in (3, 4):
        raise ValueError(f"{what} must be (Z, Y, X) or (n, Z, Y, X), got shape {shape}")
    return (1,) + shape if len(shape) == 3 else shape


def _mask(mask, dev, n):
    """None stays None (the entry points take NULL); otherwise flat uint8 0 / 1."""
    import torch

    if mask is None:
        return None
    m = mask if is_tensor(mask) else torch.from_numpy(np.ascontiguousarray(np.asarray(mask) != 0).view(np.uint8))
    m = (m != 0).to(dev, torch.uint8).contiguous().reshape(-1)
    if m.numel() != n:
        raise ValueError(f"a stack mask has {m.numel()} elements, its stack has {n}")
    return m


def _forward(lib, x, hr_shape, n_vol, B, box, pid, rel, y, mask, lr_shape, out, n_out):
    """Queue t2fit_sr_forward_dev on flat device tensors (None: NULL)."""
    ptr = lambda t: None if t is None else t.data_ptr()
    radius = (C.c_int32 * 3)(*box[1])
    check(lib.t2fit_sr_forward_dev(ptr(x), *hr_shape, n_vol, _doubles(B), _doubles(box[0]), radius, pid, float(rel), ptr(y),
                                   ptr(mask), *lr_shape, ptr(out), ptr(n_out), current_stream()))


def _adjoint(lib, r, n_list, masks, lr_shapes, B, pids, rels, x, tau, out, hr_shape, n_vol):
    """Queue t2fit_sr_adjoint_dev on flat device tensors; ``masks`` is a list that may hold None."""
    n_s = len(r)
    ptrs = lambda ts: (C.c_void_p * n_s)(*[None if t is None else t.data_ptr() for t in ts])
    check(lib.t2fit_sr_adjoint_dev(n_s, ptrs(r), ptrs(n_list), ptrs(masks), (C.c_int32 * (3 * n_s))(*[v for s in lr_shapes for v in s]),
                                   _doubles(np.concatenate([np.asarray(b, np.float64).ravel() for b in B])),
                                   (C.c_int32 * n_s)(*pids), _doubles(rels), None if x is None else x.data_ptr(), float(tau),
                                   out.data_ptr(), *hr_shape, n_vol, current_stream()))


def sr_forward(x, B, lr_shape, *, profile="box", rel_thickness=1.0, y=None, mask=None, hr_shape=None, device=0):
    """One stack of the acquisition operator on the GPU: ``(out, N)`` as :func:`_sr.forward` defines them, bit for bit.
    ``x``: float32 ``(Z, Y, X)`` or ``(n, Z, Y, X)`` on the high-resolution grid (None with ``hr_shape``: the weights only,
    ``out`` is None); ``B``: 3 x 4 from :func:`_resample.index_affine` (grid index -> stack index); ``rel_thickness``: slice
    thickness / slice spacing; ``y`` like the result: the residual ``A x - y``; ``mask``: the samples that count.  numpy in,
    numpy out; CUDA tensor in, tensors out (asynchronous on the current stream).  ``N`` is float64 ``lr_shape``."""
    import torch

    lib = require(*_abi.SR_SYMBOLS)
    pid = _sr._profile_id(profile)
    _sr.profile_params(pid, rel_thickness)
    lr_shape = tuple(int(v) for v in lr_shape)
    if len(lr_shape) != 3:
        raise ValueError("lr_shape is (Z, Y, X)")
    if x is None:
        if hr_shape is None:
            raise ValueError("the weights alone (x=None) need hr_shape")
        shape, is_t = (1,) + tuple(int(v) for v in hr_shape), False
    else:
        shape, is_t = _shape4(x, "x"), is_tensor(x)
    n_vol, n_l = shape[0], int(np.prod(lr_shape))
    b = np.asarray(B, np.float64).reshape(3, 4)
    box = sr_box(b, pid, rel_thickness)
    dev = pick_device((x, y, mask), device)
    with torch.cuda.device(dev):
        xt = None if x is None else flat(x, dev)
        yt = None if y is None else flat(y, dev, n_vol * n_l, "y")
        mt = _mask(mask, dev, n_l)
        n_out = torch.empty(lr_shape, dtype=torch.float64, device=dev)
        out = None if x is None else torch.empty((n_vol,) + lr_shape, dtype=torch.float32, device=dev)
        _forward(lib, xt, shape[-3:], n_vol, b, box, pid, rel_thickness, yt, mt, lr_shape, out, n_out)
        release(xt, yt, mt)
    if out is not None and len(x.shape) == 3:
        out = out[0]
    host = (lambda t: t) if is_t else (lambda t: None if t is None else t.cpu().numpy())
    return host(out), host(n_out)


def sr_adjoint(r, N, B, profile, rel_thickness, hr_shape, *, masks=None, x=None, tau=0.0, device=0):
    """``sum_s A_s^T r_s`` (or ``x - tau`` times it) on the grid ``hr_shape`` as :func:`_sr.adjoint` defines it, bit for
    bit: lists over 1 to 6 stacks of residuals, of the normalisers :func:`sr_forward` returned and of affines; ``profile`` and
    ``rel_thickness`` per stack or one for all.  numpy in, numpy out; CUDA tensors in, tensor out."""
    import torch

    lib = require(*_abi.SR_SYMBOLS)
    n_s = len(r)
    if not 1 <= n_s <= _abi.SR_MAX_STACKS or len(N) != n_s or len(B) != n_s:
        raise ValueError(f"between 1 and {_abi.SR_MAX_STACKS} stacks with one N and one B each")
    pids = [_sr._profile_id(p) for p in ([profile] * n_s if isinstance(profile, (str, int)) else profile)]
    rels = [float(v) for v in ([rel_thickness] * n_s if np.ndim(rel_thickness) == 0 else rel_thickness)]
    for p, t in zip(pids, rels):
        _sr.profile_params(p, t)
    masks = [None] * n_s if masks is None else list(masks)
    shapes = [_shape4(v, "a residual") for v in r]
    if len({s[0] for s in shapes}) != 1:
        raise ValueError("the residuals differ in their number of volumes")
    n_vol = shapes[0][0]
    hr_shape = tuple(int(v) for v in hr_shape)
    is_t = is_tensor(r[0])
    dev = pick_device(list(r) + [x], device)
    with torch.cuda.device(dev):
        rt = [flat(v, dev) for v in r]
        nt = [flat(v, dev, int(np.prod(s[-3:])), "N", dtype="float64") for v, s in zip(N, shapes)]
        mt = [_mask(m, dev, int(np.prod(s[-3:]))) for m, s in zip(masks, shapes)]
        xt = None if x is None else flat(x, dev, n_vol * int(np.prod(hr_shape)), "x")
        out = torch.empty((n_vol,) + hr_shape, dtype=torch.float32, device=dev)
        _adjoint(lib, rt, nt, mt, [s[-3:] for s in shapes], B, pids, rels, xt, tau, out, hr_shape, n_vol)
        release(xt, *rt, *nt, *mt)
    if len(r[0].shape) == 3:
        out = out[0]
    return out if is_t else out.cpu().numpy()


# ---- a rigid pose per slice ----------------------------------------------------------------------------------------------
def sr_slice_table(B_slices, profile="box", rel_thickness=1.0):
    """The slice table of t2fit_sr_slice_table_host for a stack whose slice k has the affine ``B_slices[k]`` (``(lz, 3,
    4)``): a uint8 numpy array of ``208 lz`` bytes (B, Binv, radii per slice; include/t2fit.h has the layout).  Host
    arithmetic; refuses what t2fit_sr_plan_host refuses, for every slice."""
    lib = require(*_abi.SR_SLICE_SYMBOLS)
    b = np.ascontiguousarray(B_slices, np.float64)
    if b.ndim != 3 or b.shape[1:] != (3, 4) or b.shape[0] < 1:
        raise ValueError(f"one 3 x 4 affine per slice, (lz, 3, 4), got shape {b.shape}")
    pid = _sr._profile_id(profile)
    _sr.profile_params(pid, rel_thickness)
    need = C.c_size_t(0)
    check(lib.t2fit_sr_slice_table_bytes(len(b), C.byref(need)))
    table = np.zeros(need.value, np.uint8)
    check(lib.t2fit_sr_slice_table_host(len(b), b.ctypes.data_as(C.POINTER(C.c_double)), pid, float(rel_thickness),
                                        table.ctypes.data_as(C.c_void_p), need.value))
    return table


def _table(table, dev, lz):
    """A slice table on the device (8-byte aligned: a fresh allocation); ``table``: bytes from :func:`sr_slice_table`."""
    import torch

    t = table if is_tensor(table) else torch.from_numpy(np.ascontiguousarray(table, np.uint8))
    t = t.to(dev).contiguous().reshape(-1)
    if t.dtype != torch.uint8 or t.numel() != _abi.SR_SLICE_RECORD_BYTES * lz:
        raise ValueError(f"a slice table of {lz} slices is {_abi.SR_SLICE_RECORD_BYTES * lz} bytes of uint8")
    return t


def _forward_slices(lib, x, hr_shape, n_vol, table, pid, rel, y, mask, lr_shape, out, n_out):
    """Queue t2fit_sr_slice_forward_dev on flat device tensors (None: NULL)."""
    ptr = lambda t: None if t is None else t.data_ptr()
    check(lib.t2fit_sr_slice_forward_dev(ptr(x), *hr_shape, n_vol, table.data_ptr(), pid, float(rel), ptr(y), ptr(mask), *lr_shape,
                                         ptr(out), ptr(n_out), current_stream()))


def _adjoint_slices(lib, r, n_list, masks, tables, lr_shapes, pids, rels, x, tau, out, hr_shape, n_vol):
    """Queue t2fit_sr_slice_adjoint_dev on flat device tensors; ``masks`` is a list that may hold None."""
    n_s = len(r)
    ptrs = lambda ts: (C.c_void_p * n_s)(*[None if t is None else t.data_ptr() for t in ts])
    check(lib.t2fit_sr_slice_adjoint_dev(n_s, ptrs(r), ptrs(n_list), ptrs(masks), ptrs(tables),
                                         (C.c_int32 * (3 * n_s))(*[v for s in lr_shapes for v in s]), (C.c_int32 * n_s)(*pids),
                                         _doubles(rels), None if x is None else x.data_ptr(), float(tau), out.data_ptr(), *hr_shape,
                                         n_vol, current_stream()))


def sr_forward_slices(x, B_slices, lr_shape, *, profile="box", rel_thickness=1.0, y=None, mask=None, hr_shape=None, device=0):
    """:func:`sr_forward` with an affine per slice (``B_slices``: ``(lz, 3, 4)``), as :func:`_sr.forward_slices` defines it,
    bit for bit: sample ``j`` takes its weights from ``B_slices[j_z]``."""
    import torch

    lib = require(*_abi.SR_SLICE_SYMBOLS)
    pid = _sr._profile_id(profile)
    lr_shape = tuple(int(v) for v in lr_shape)
    if len(lr_shape) != 3:
        raise ValueError("lr_shape is (Z, Y, X)")
    table = sr_slice_table(_sr._slice_affine_list(B_slices, lr_shape[0]), pid, rel_thickness)
    if x is None:
        if hr_shape is None:
            raise ValueError("the weights alone (x=None) need hr_shape")
        shape, is_t = (1,) + tuple(int(v) for v in hr_shape), False
    else:
        shape, is_t = _shape4(x, "x"), is_tensor(x)
    n_vol, n_l = shape[0], int(np.prod(lr_shape))
    dev = pick_device((x, y, mask), device)
    with torch.cuda.device(dev):
        xt = None if x is None else flat(x, dev)
        yt = None if y is None else flat(y, dev, n_vol * n_l, "y")
        mt = _mask(mask, dev, n_l)
        tt = _table(table, dev, lr_shape[0])
        n_out = torch.empty(lr_shape, dtype=torch.float64, device=dev)
        out = None if x is None else torch.empty((n_vol,) + lr_shape, dtype=torch.float32, device=dev)
        _forward_slices(lib, xt, shape[-3:], n_vol, tt, pid, rel_thickness, yt, mt, lr_shape, out, n_out)
        release(xt, yt, mt, tt)
    if out is not None and len(x.shape) == 3:
        out = out[0]
    host = (lambda t: t) if is_t else (lambda t: None if t is None else t.cpu().numpy())
    return host(out), host(n_out)


def sr_adjoint_slices(r, N, B_slices, profile, rel_thickness, hr_shape, *, masks=None, x=None, tau=0.0, device=0):
    """:func:`sr_adjoint` with an affine per slice (``B_slices[s]``: ``(lz_s, 3, 4)``), as :func:`_sr.adjoint_slices` defines
    it, bit for bit: within a stack every slice in ascending index, culled per tile of voxels on the device."""
    import torch

    lib = require(*_abi.SR_SLICE_SYMBOLS)
    n_s = len(r)
    if not 1 <= n_s <= _abi.SR_MAX_STACKS or len(N) != n_s or len(B_slices) != n_s:
        raise ValueError(f"between 1 and {_abi.SR_MAX_STACKS} stacks with one N and one list of slice affines each")
    pids = [_sr._profile_id(p) for p in ([profile] * n_s if isinstance(profile, (str, int)) else profile)]
    rels = [float(v) for v in ([rel_thickness] * n_s if np.ndim(rel_thickness) == 0 else rel_thickness)]
    masks = [None] * n_s if masks is None else list(masks)
    shapes = [_shape4(v, "a residual") for v in r]
    if len({s[0] for s in shapes}) != 1:
        raise ValueError("the residuals differ in their number of volumes")
    tables = [sr_slice_table(_sr._slice_affine_list(b, s[-3]), p, t) for b, s, p, t in zip(B_slices, shapes, pids, rels)]
    n_vol = shapes[0][0]
    hr_shape = tuple(int(v) for v in hr_shape)
    is_t = is_tensor(r[0])
    dev = pick_device(list(r) + [x], device)
    with torch.cuda.device(dev):
        rt = [flat(v, dev) for v in r]
        nt = [flat(v, dev, int(np.prod(s[-3:])), "N", dtype="float64") for v, s in zip(N, shapes)]
        mt = [_mask(m, dev, int(np.prod(s[-3:]))) for m, s in zip(masks, shapes)]
        tt = [_table(t, dev, s[-3]) for t, s in zip(tables, shapes)]
        xt = None if x is None else flat(x, dev, n_vol * int(np.prod(hr_shape)), "x")
        out = torch.empty((n_vol,) + hr_shape, dtype=torch.float32, device=dev)
        _adjoint_slices(lib, rt, nt, mt, tt, [s[-3:] for s in shapes], pids, rels, xt, tau, out, hr_shape, n_vol)
        release(xt, *rt, *nt, *mt, *tt)
    if len(r[0].shape) == 3:
        out = out[0]
    return out if is_t else out.cpu().numpy()


# ---- outlier weighting ---------------------------------------------------------------------------------------------------
def robust_struct(params):
    """``t2fit_sr_robust_params`` from the checked dict of :func:`_sr.robust_params`."""
    return _abi.T2FitSrRobustParams(params["slice_threshold"], params["huber"], params["sigma_floor"], params["min_count"], 0)


def _robust(lib, r, n_list, masks, lr_shapes, n_vol, par, sums, weights, sigma2):
    """Queue t2fit_sr_robust_dev on flat device tensors; ``masks`` is a list that may hold None."""
    n_s = len(r)
    ptrs = lambda ts: (C.c_void_p * n_s)(*[None if t is None else t.data_ptr() for t in ts])
    check(lib.t2fit_sr_robust_dev(n_s, ptrs(r), ptrs(n_list), ptrs(masks), (C.c_int32 * (3 * n_s))(*[v for s in lr_shapes for v in s]),
                                  n_vol, C.byref(par), sums.data_ptr(), weights.data_ptr(), sigma2.data_ptr(), current_stream()))


def sr_robust_weights(r, N, *, masks=None, device=0, **params):
    """The outlier weighting of the robust loop on the residuals of 1 to 6 stacks, as :func:`_sr.robust_step` defines it, bit
    for bit: ``r`` a list of float32 residuals ``(lz, ly, lx)`` or ``(n, lz, ly, lx)``, ``N`` the normalisers of
    :func:`sr_forward`, ``masks`` a list that may hold None; ``params``: ``slice_threshold``, ``huber``, ``min_count``,
    ``sigma_floor`` (:data:`_sr.ROBUST_DEFAULTS`).  Returns ``(weighted r, slice weights, sigma2, sums)``: lists over the
    stacks of residuals like ``r`` (the inputs stay as they are) and of ``(n, lz)`` float64 weights, ``(n,)`` and
    ``(n, n_slices, 2)`` float64.  numpy in, numpy out; CUDA tensors in, tensors out (asynchronous on the current stream)."""
    import torch

    lib = require(*_abi.SR_ROBUST_SYMBOLS)
    par = robust_struct(_sr.robust_params(params or True))
    n_s = len(r)
    if not 1 <= n_s <= _abi.SR_MAX_STACKS or len(N) != n_s:
        raise ValueError(f"between 1 and {_abi.SR_MAX_STACKS} stacks with one N each")
    masks = [None] * n_s if masks is None else list(masks)
    shapes = [_shape4(v, "a residual") for v in r]
    if len({s[0] for s in shapes}) != 1:
        raise ValueError("the residuals differ in their number of volumes")
    n_vol, n_slices = shapes[0][0], sum(s[1] for s in shapes)
    if n_slices > _abi.SR_ROBUST_MAX_SLICES:
        raise ValueError(f"at most {_abi.SR_ROBUST_MAX_SLICES} slices in total, got {n_slices}")
    is_t = is_tensor(r[0])
    dev = pick_device(list(r), device)
    with torch.cuda.device(dev):
        rt = [flat(v, dev).clone() for v in r]
        nt = [flat(v, dev, int(np.prod(s[-3:])), "N", dtype="float64") for v, s in zip(N, shapes)]
        mt = [_mask(m, dev, int(np.prod(s[-3:]))) for m, s in zip(masks, shapes)]
        sums = torch.empty((n_vol, n_slices, 2), dtype=torch.float64, device=dev)
        weights = torch.empty((n_vol, n_slices), dtype=torch.float64, device=dev)
        sigma2 = torch.empty(n_vol, dtype=torch.float64, device=dev)
        _robust(lib, rt, nt, mt, [s[-3:] for s in shapes], n_vol, par, sums, weights, sigma2)
        release(*nt, *mt)
    edges = np.cumsum([0] + [s[1] for s in shapes])
    out = [t.reshape(tuple(v.shape)) for t, v in zip(rt, r)]
    per_stack = [weights[:, edges[s]:edges[s + 1]] for s in range(n_s)]
    if is_t:
        return out, [w.contiguous() for w in per_stack], sigma2, sums
    host = lambda t: t.cpu().numpy()
    return [host(t) for t in out], [np.ascontiguousarray(host(w)) for w in per_stack], host(sigma2), host(sums)


def reconstruct_sr(stacks, geoms, *, fixed="ax", res=1.0, transforms=None, thickness=None, profile="box",
                   weight=_sr.DEFAULT_WEIGHT, n_iter=_sr.DEFAULT_N_ITER, prox_iter=_sr.DEFAULT_PROX_ITER, stack_masks=None,
                   x0=None, return_info=False, device=0, slice_transforms=None, robust=None, tv="channel"):
    """TV-regularised super-resolution reconstruction of 1 to 6 thick-slice stacks on the GPU.  Each slice is modelled as
    the slice-profile average of the ``res`` mm volume x on the ``fixed`` stack's isotropic grid, and per echo

        1/2 sum_s ||A_s x - y_s||^2 + weight * TV(x)

    is reduced by ``n_iter`` proximal-gradient steps from ``x0`` (default: the averaged merge of
    :func:`reconstruct_stacks` when the stacks are ax, cor and sag, else the fixed stack's own linear resample); the prox is
    :func:`denoise_tv` in 3-D with ``prox_iter`` iterations.  ``weight`` is in intensity units of the stacks (0: plain
    iterative back-projection).  ``stacks`` / ``geoms``: {name: float32 ``(nTE, Z, Y, X)`` or ``(Z, Y, X)``} and their
    geometries; ``transforms``: {moving stack: 4 x 4, fixed point -> moving point}; ``thickness``: slice thickness in mm, one
    number or {name: mm} (default: the slice spacing); ``profile``: ``'box'`` or ``'bspline3'``; ``stack_masks``: {name: the
    samples that count, ``(Z, Y, X)``}.  ``slice_transforms``: {stack name: ``(lz, 4, 4)``}, a rigid pose per slice (fixed
    point -> stack point) that takes the place of the stack's transform for that slice; the fixed stack may have an entry,
    stacks without one carry their stack transform on every slice.  Then the normalisers, the step size and the loop run on
    the slice operators (:func:`sr_forward_slices`, :func:`sr_adjoint_slices`) and ``x0`` stays the merge; None takes the
    stack-wise path.
    Returns ``(echoes, header)`` like :func:`reconstruct_stacks`: a float32 CUDA tensor ``(nTE, Z, Y, X)`` and a
    ``nifti.Image`` over an empty array with the grid's geometry; with ``return_info`` also ``{"tau", "column_max", "N"}``.
    ``robust`` (None, True for :data:`_sr.ROBUST_DEFAULTS`, or a dict of them): outlier weighting.  Every iteration
    multiplies its residuals by a weight per slice and a Huber weight per sample, both scaled by a robust noise estimate per
    echo (:func:`sr_robust_weights`, one more launch group, still no synchronisation); the info then also holds
    ``"slice_weights"`` (one float64 ``(nTE, lz)`` tensor per stack), ``"sigma2"`` (``(nTE,)``) and ``"robust_sums"``
    (``(nTE, n_slices, 2)``: count and sum of squares per slice) of the last iteration.  None launches none of it.
    ``tv``: ``"channel"`` (every echo's prox on its own) or ``"joint"``: the prox is the vector-valued TV across the echoes
    (``t2fit_tv_joint_denoise_dev`` in 3-D, one problem, the same ``w = tau * weight``, ``eps = 0`` and ``prox_iter``), so
    all echoes of the volume share one edge set; with one echo it equals ``"channel"``.
    The step size is read back once before the loop (one synchronisation); the loop itself queues 3 + stacks launch groups
    per iteration and does not synchronise.  :func:`_sr.reconstruct_sr` states the definition in numpy; same bits."""
    import torch

    from . import nifti

    robust = _sr.robust_params(robust)
    if tv not in ("channel", "joint"):
        raise ValueError(f"tv must be 'channel' or 'joint', got {tv!r}")
    lib = require(*(_abi.SR_SYMBOLS + _abi.TV_SYMBOLS + (() if slice_transforms is None else _abi.SR_SLICE_SYMBOLS)
                    + (() if robust is None else _abi.SR_ROBUST_SYMBOLS) + (_abi.TVJ_SYMBOLS if tv == "joint" else ())))
    tv_bytes, tv_call = ((lib.t2fit_tv_joint_workspace_bytes, lib.t2fit_tv_joint_denoise_dev) if tv == "joint" else
                         (lib.t2fit_tv_workspace_bytes, lib.t2fit_tv_denoise_dev))
    if not (float(weight) >= 0.0 and np.isfinite(weight)) or int(n_iter) < 0 or int(prox_iter) < 1:
        raise ValueError("weight must be finite and >= 0, n_iter >= 0, prox_iter >= 1")
    pid = _sr._profile_id(profile)
    names = [o for o in geoms if o in stacks]
    shapes = {o: _shape4(stacks[o], f"stack {o!r}") for o in names}
    if len({len(stacks[o].shape) for o in names}) > 1 or len({s[0] for s in shapes.values()}) > 1:
        raise ValueError(f"the stacks must all be (Z, Y, X) or all (nTE, Z, Y, X) with one number of echoes, got "
                         f"{ {o: tuple(stacks[o].shape) for o in names} }")
    g = {o: _resample.as_geometry(geoms[o], shapes[o][-3:]) for o in names}
    order, hi, B, rels = _sr.sr_plan(g, fixed, res, transforms, thickness)
    n_s, n_vol, hr_shape = len(order), shapes[order[0]][0], hi.shape
    lr_shapes = [shapes[o][-3:] for o in order]
    if slice_transforms is None:
        boxes, tables = [sr_box(B[s], pid, rels[s]) for s in range(n_s)], None
    else:
        slices = _sr.slice_plan(order, hi, g, B, lr_shapes, slice_transforms)
        boxes, tables = None, [sr_slice_table(slices[s], pid, rels[s]) for s in range(n_s)]
    dev = pick_device([stacks[o] for o in order], device)
    lo_size = (C.c_int32 * (3 * n_s))(*[v for s in lr_shapes for v in s])
    need = C.c_size_t(0)
    check(lib.t2fit_sr_workspace_bytes(n_s, lo_size, *hr_shape, n_vol, C.byref(need)))
    robust_need, n_slices = C.c_size_t(0), sum(s[0] for s in lr_shapes)
    if robust is not None:
        check(lib.t2fit_sr_robust_workspace_bytes(n_s, lo_size, n_vol, C.byref(robust_need)))
        robust_par = robust_struct(robust)
    n_h = int(np.prod(hr_shape))
    with torch.cuda.device(dev):
        y = [flat(stacks[o], dev) for o in order]
        masks = [_mask(None if stack_masks is None else stack_masks.get(o), dev, int(np.prod(s))) for o, s in zip(order, lr_shapes)]
        # x_0 before the workspace is carved: the merge has a workspace of its own
        if x0 is not None:
            x = flat(x0, dev, n_vol * n_h, "x0").clone()
        elif sorted(order) == sorted(_resample.ORIENTATIONS):
            x = reconstruct_stacks({o: stacks[o] for o in order}, g, fixed=fixed, res=res, transforms=transforms, device=dev.index)[0].reshape(-1)
        else:
            x = resample_volume(y[0].reshape((n_vol,) + lr_shapes[0]), g[order[0]], like=hi)[0].reshape(-1)
        ws, base = workspace(need.value + robust_need.value, dev)
        off = base - ws.data_ptr()

        def carve(nbytes, dtype):
            nonlocal off
            t = ws[off:off + nbytes].view(dtype)
            off += (nbytes + 255) // 256 * 256
            return t

        z = carve(4 * n_vol * n_h, torch.float32)
        N, r = [], []
        for s in lr_shapes:
            N.append(carve(8 * int(np.prod(s)), torch.float64))
            r.append(carve(4 * n_vol * int(np.prod(s)), torch.float32))
        assert off - (base - ws.data_ptr()) == need.value
        if robust is not None:
            sums = carve(16 * n_vol * n_slices, torch.float64)
            q = carve(8 * n_vol * n_slices, torch.float64)
            sigma2 = carve(8 * n_vol, torch.float64)
            assert off - (base - ws.data_ptr()) == need.value + robust_need.value
        if tables is None:
            def fwd(s, xs, nv, ys, ms, out, n_out):
                _forward(lib, xs, hr_shape, nv, B[s], boxes[s], pid, rels[s], ys, ms, lr_shapes[s], out, n_out)

            def adj(idx, rs, xs, step, out, nv):
                _adjoint(lib, rs, [N[s] for s in idx], [masks[s] for s in idx], [lr_shapes[s] for s in idx], [B[s] for s in idx],
                         [pid] * len(idx), [rels[s] for s in idx], xs, step, out, hr_shape, nv)
        else:
            tables = [_table(t, dev, lr_shapes[s][0]) for s, t in enumerate(tables)]  # uploaded once, reused across the loop

            def fwd(s, xs, nv, ys, ms, out, n_out):
                _forward_slices(lib, xs, hr_shape, nv, tables[s], pid, rels[s], ys, ms, lr_shapes[s], out, n_out)

            def adj(idx, rs, xs, step, out, nv):
                _adjoint_slices(lib, rs, [N[s] for s in idx], [masks[s] for s in idx], [tables[s] for s in idx],
                                [lr_shapes[s] for s in idx], [pid] * len(idx), [rels[s] for s in idx], xs, step, out, hr_shape, nv)
        # the normalisers, then tau from the per-stack column sums A_s^T 1 (z and r_s serve as scratch)
        col_max = []
        for s in range(n_s):
            fwd(s, None, 1, None, None, None, N[s])
            ones = r[s][:N[s].numel()]
            ones.copy_(((N[s] > 0) if masks[s] is None else (N[s] > 0) & (masks[s] != 0)).to(torch.float32))
            adj([s], [ones], None, 0.0, z, 1)
            col_max.append(z[:n_h].max())
        col_max = [float(v) for v in torch.stack(col_max).tolist()]  # the one read-back
        tau = _sr.step_size(col_max)
        if float(weight) > 0.0:
            par = tv_params(tau * float(weight), 0.0, int(prox_iter), 3, "f32")
            tv_need = C.c_size_t(0)
            check(tv_bytes(C.byref(par), n_vol, *hr_shape, C.byref(tv_need)))
            tv_ws, tv_ptr = workspace(tv_need.value, dev)
        stream = current_stream()
        for _ in range(int(n_iter)):
            for s in range(n_s):
                fwd(s, x, n_vol, y[s], masks[s], r[s], None)
            if robust is not None:
                _robust(lib, r, N, masks, lr_shapes, n_vol, robust_par, sums, q, sigma2)
            if float(weight) > 0.0:
                adj(range(n_s), r, x, tau, z, n_vol)
                check(tv_call(C.byref(par), z.data_ptr(), x.data_ptr(), n_vol, *hr_shape, tv_ptr, tv_need.value, None, None, stream))
            else:
                adj(range(n_s), r, x, tau, x, n_vol)
        info = {"tau": tau, "column_max": col_max, "N": [n.clone().reshape(s) for n, s in zip(N, lr_shapes)]} if return_info else None
        if return_info and robust is not None:
            ran = int(n_iter) > 0
            edges = np.cumsum([0] + [s[0] for s in lr_shapes])
            table = q.reshape(n_vol, n_slices)
            info["slice_weights"] = [table[:, edges[s]:edges[s + 1]].clone() for s in range(n_s)] if ran else None
            info["sigma2"] = sigma2.clone() if ran else None
            info["robust_sums"] = sums.reshape(n_vol, n_slices, 2).clone() if ran else None
        if float(weight) > 0.0:
            release(tv_ws)
        release(ws, *y, *[m for m in masks if m is not None], *(tables or []))
    out = x.reshape((n_vol,) + hr_shape)
    header = nifti.Image(np.zeros((0, 0, 0), np.float32), hi.GetSpacing(), hi.GetOrigin(), hi.GetDirection())
    return (out, header, info) if return_info else (out, header)


def reconstruct_svr(stacks, geoms, *, rounds=2, echo=0, slice_masks=None, volume_mask=None, max_iter=_svr.MAX_ITER, step=_svr.STEP,
                    min_step=_svr.MIN_STEP, min_count=_svr.MIN_COUNT, **sr):
    """Motion-corrected super-resolution: the slice poses :func:`reconstruct_sr` takes are found here, not given.  From the
    merge (``reconstruct_sr`` with no iteration), ``rounds`` times: every slice of every stack is registered onto echo
    ``echo`` of the current volume (``t2map.register.register_slices``, warm-started from the last round; ``slice_masks``:
    {name: ``(Z, Y, X)``} of the registration, None: ``build_mask`` of the stack; ``volume_mask``, ``max_iter``, ``step``,
    ``min_step``, ``min_count`` are its arguments) and the volume is reconstructed again with the poses found.  Every other
    keyword is :func:`reconstruct_sr`'s (``device`` too); ``slice_transforms`` and ``return_info`` are refused.  Returns
    ``(echoes, header, found)``: ``found`` is the :class:`_svr.SliceRegistration` of the last round, ``found.transforms``
    what ``slice_transforms=`` and ``recon.py --sr_slice_transforms`` read.  :func:`_svr.reconstruct_svr` states it in numpy;
    same bits."""
    from ._gpu_register import register_slices

    _svr.check_options(max_iter, step, min_step, min_count)
    device = sr.get("device", 0)

    def register(*args, **kw):
        return register_slices(*args, device=device, **kw)

    return _svr.drive(reconstruct_sr, register, stacks, geoms, rounds, echo, slice_masks, volume_mask,
                      dict(max_iter=max_iter, step=step, min_step=min_step, min_count=min_count), sr)
