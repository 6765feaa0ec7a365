"""Atlas-prior EM tissue segmentation on the GPU; :mod:`fetal_t2mapping_amd._seg` states every step in numpy and holds the
loop, which this module runs with device steps."""
import ctypes as C
import functools

import numpy as np

from . import _abi, _seg
from ._gpu import check_out, current_stream, flat, is_tensor, mask_u8, pick_device, release, require, workspace
from ._lib import check

_I32P, _F64P = C.POINTER(C.c_int32), C.POINTER(C.c_double)


def seg_params(sigma=2.0, beta=0.5, prior_floor=1e-3, var_floor=1e-6, n_iter=15, tol=0.0):
    """The keywords of :func:`segment_em` (and ``sigma`` of :func:`priors_from_labels`) with their defaults, as a dict.  The
    defaults come from a sweep on one synthetic phantom and nothing else."""
    return dict(sigma=sigma, beta=float(beta), prior_floor=float(prior_floor), var_floor=float(var_floor), n_iter=int(n_iter),
                tol=float(tol))


def _planes(a, who, what):
    shape = tuple(int(v) for v in a.shape)
    if len(shape) != 4:
        raise ValueError(f"{who} needs {what} as (n, Z, Y, X), got shape {shape}")
    return shape


def _host(t, like):
    return t if is_tensor(like) else t.cpu().numpy()


def _i32(values):
    arr = np.ascontiguousarray(values, np.int32)
    return arr, arr.ctypes.data_as(_I32P)


def _ws(lib, K, Cn, vol, dev):
    need = C.c_size_t(0)
    check(lib.t2fit_seg_workspace_bytes(K, Cn, *vol, C.byref(need)))
    return workspace(need.value, dev)


def effective_mask(y, mask, device=0):
    """``M`` as a uint8 0 / 1 volume: ``mask != 0`` (None: everywhere) and every channel of ``y`` ``(C, Z, Y, X)`` finite."""
    import torch

    lib = require(*_abi.SEG_SYMBOLS)
    Cn, nz, ny, nx = _planes(y, "effective_mask", "y")
    dev = pick_device((y, mask), device)
    n = nz * ny * nx
    src = flat(y, dev)
    msk = None if mask is None else mask_u8(mask, dev, n)
    out = torch.empty(n, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.t2fit_seg_mask_dev(src.data_ptr(), None if msk is None else msk.data_ptr(), Cn, n, out.data_ptr(), current_stream()))
        release(src, msk)
    return _host(out.reshape(nz, ny, nx), y)


def priors_from_labels(labels, classes, sigma=2.0, *, out=None, device=0):
    """``(K, Z, Y, X)`` float32 spatial priors: the one-hot images ``labels == classes[k]`` blurred by a Gaussian of ``sigma``
    voxels (a scalar, or z, y, x), truncated at 4 sigma, zero beyond the volume.  ``labels``: an integer ``(Z, Y, X)`` numpy
    array (numpy result) or CUDA tensor (tensor result, asynchronous on the current stream)."""
    import torch

    lib = require(*_abi.SEG_SYMBOLS)
    classes = _seg._classes(classes)
    wz, wy, wx = _seg._axis_taps(sigma)
    vol = tuple(int(v) for v in labels.shape)
    if len(vol) != 3:
        raise ValueError(f"priors_from_labels needs labels as (Z, Y, X), got shape {vol}")
    K = len(classes)
    dev = pick_device((labels,), device)
    lab = flat(labels, dev, dtype="int32")
    if out is None:
        dst = torch.empty((K,) + vol, dtype=torch.float32, device=dev)
    else:
        check_out(out, torch.float32, (K,) + vol, dev)
        dst = out
    cls, cls_p = _i32(classes)
    with torch.cuda.device(dev):
        ws, ws_ptr = _ws(lib, K, 1, vol, dev)
        check(lib.t2fit_seg_priors_dev(lab.data_ptr(), cls_p, K, *vol, wz.ctypes.data_as(_F64P), (len(wz) - 1) // 2,
                                       wy.ctypes.data_as(_F64P), (len(wy) - 1) // 2, wx.ctypes.data_as(_F64P), (len(wx) - 1) // 2,
                                       dst.data_ptr(), ws_ptr, current_stream()))
        release(ws, lab)
    return _host(dst, labels)


def normalise_priors(prior, mask, floor=1e-3, *, device=0):
    """``pi`` from the priors, the mask and the floor (``_seg.normalise_priors``)."""
    import torch

    lib = require(*_abi.SEG_SYMBOLS)
    K, nz, ny, nx = _planes(prior, "normalise_priors", "prior")
    dev = pick_device((prior, mask), device)
    n = nz * ny * nx
    src, msk = flat(prior, dev), mask_u8(mask, dev, n)
    dst = torch.empty(K * n, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(lib.t2fit_seg_normalise_dev(src.data_ptr(), msk.data_ptr(), K, n, float(floor), dst.data_ptr(), current_stream()))
        release(src, msk)
    return _host(dst.reshape(K, nz, ny, nx), prior)


def _effective(y, mask, dev, n, trusted):
    """The flat device ``M`` of a step: of a step called on its own the raw mask is not trusted to leave out non-finite
    voxels; the loop hands its steps the ``M`` it made (``trusted``), which is taken as it is."""
    if trusted:
        return mask_u8(mask, dev, n)
    return effective_mask(y, mask).reshape(-1)


def moment_sums(p, y, mask, *, device=0, mask_is_effective=False):
    """``(K, 1 + C + C (C + 1) / 2)`` float64 numpy array: the moments of every class over ``M`` in the fixed tree of
    ``_seg.moment_sums``, to which it is equal bit for bit.  Synchronises (the host builds the class model from them).
    ``mask_is_effective``: ``mask`` is already ``M`` (what :func:`effective_mask` returned) and is not formed again."""
    import torch

    lib = require(*_abi.SEG_SYMBOLS)
    K, nz, ny, nx = _planes(p, "moment_sums", "p")
    Cn = _planes(y, "moment_sums", "y")[0]
    if tuple(y.shape[1:]) != (nz, ny, nx):
        raise ValueError("moment_sums: p and y are not on one grid")
    dev = pick_device((p, y, mask), device)
    n = nz * ny * nx
    with torch.cuda.device(dev):
        pv, yv = flat(p, dev, K * n, "p"), flat(y, dev)
        msk = _effective(yv.reshape(Cn, nz, ny, nx), mask, dev, n, mask_is_effective)
        out = torch.empty(K * _seg.n_moments(Cn), dtype=torch.float64, device=dev)
        ws, ws_ptr = _ws(lib, K, Cn, (nz, ny, nx), dev)
        check(lib.t2fit_seg_sums_dev(pv.data_ptr(), yv.data_ptr(), msk.data_ptr(), K, Cn, nz, ny, nx, out.data_ptr(), ws_ptr,
                                     current_stream()))
        release(ws, pv, yv, msk)
        return out.cpu().numpy().reshape(K, _seg.n_moments(Cn))


def e_step(p_old, pi, y, mask, model, beta, *, out=None, device=0, mask_is_effective=False):
    """One E-step (``_seg.e_step``) into a new buffer, or into ``out`` (which must not be ``p_old``).  ``model``: a
    ``_seg.SegModel`` or the ``(rows, live)`` pair of ``_seg.pack_model``.  Within 1 float32 ulp of the statement.
    ``mask_is_effective``: as in :func:`moment_sums`."""
    import torch

    lib = require(*_abi.SEG_SYMBOLS)
    K, nz, ny, nx = _planes(p_old, "e_step", "p_old")
    Cn = _planes(y, "e_step", "y")[0]
    if tuple(pi.shape) != (K, nz, ny, nx) or tuple(y.shape[1:]) != (nz, ny, nx):
        raise ValueError("e_step: p_old, pi and y are not on one grid")
    rows, live = _seg.pack_model(model) if isinstance(model, _seg.SegModel) else model
    rows = np.ascontiguousarray(rows, np.float64)
    if rows.shape != (K, Cn + Cn * (Cn + 1) // 2 + 1):
        raise ValueError(f"e_step: the model has shape {rows.shape}, not (K, C + C (C + 1) / 2 + 1)")
    live, live_p = _i32(live)
    dev = pick_device((p_old, pi, y, mask), device)
    n = nz * ny * nx
    with torch.cuda.device(dev):
        po, pv, yv = flat(p_old, dev, K * n, "p_old"), flat(pi, dev, K * n, "pi"), flat(y, dev)
        msk = _effective(yv.reshape(Cn, nz, ny, nx), mask, dev, n, mask_is_effective)
        if out is None:
            dst = torch.empty((K, nz, ny, nx), dtype=torch.float32, device=dev)
        else:
            check_out(out, torch.float32, (K, nz, ny, nx), dev)
            dst = out
        check(lib.t2fit_seg_estep_dev(po.data_ptr(), pv.data_ptr(), yv.data_ptr(), msk.data_ptr(), rows.ctypes.data_as(_F64P), live_p,
                                      float(beta), K, Cn, nz, ny, nx, dst.data_ptr(), current_stream()))
        release(po, pv, yv, msk)
    return _host(dst, p_old)


def hard_labels(p, classes, mask, *, device=0):
    """int32 ``classes[first argmax_k p]`` where ``mask != 0``, 0 elsewhere."""
    import torch

    lib = require(*_abi.SEG_SYMBOLS)
    K, nz, ny, nx = _planes(p, "hard_labels", "p")
    classes = _seg._classes(classes)
    if len(classes) != K:
        raise ValueError("hard_labels: one class value per plane of p")
    dev = pick_device((p, mask), device)
    n = nz * ny * nx
    pv, msk = flat(p, dev), mask_u8(mask, dev, n)
    out = torch.empty(n, dtype=torch.int32, device=dev)
    cls, cls_p = _i32(classes)
    with torch.cuda.device(dev):
        check(lib.t2fit_seg_labels_dev(pv.data_ptr(), msk.data_ptr(), cls_p, K, n, out.data_ptr(), current_stream()))
        release(pv, msk)
    return _host(out.reshape(nz, ny, nx), p)


# the steps as the loop calls them: the mask they get is the M that effective_mask returned
DEVICE_STEPS = _seg.SegSteps(effective_mask, normalise_priors, functools.partial(moment_sums, mask_is_effective=True),
                             functools.partial(e_step, mask_is_effective=True), hard_labels)


def segment_em(y, mask, prior, classes, *, beta=0.5, prior_floor=1e-3, var_floor=1e-6, n_iter=15, tol=0.0, return_posteriors=False,
               min_island=0, device=0):
    """EM tissue segmentation on the GPU: ``_seg.segment_em``'s loop (``_seg.run_em``) with the device steps, the volumes
    staying on the device between them.  ``y``: float32 ``(C, Z, Y, X)`` (or one ``(Z, Y, X)`` volume), 1 .. 4 channels;
    ``prior``: ``(K, Z, Y, X)`` from :func:`priors_from_labels`; ``classes``: the K label values; numpy arrays (numpy results)
    or CUDA tensors (tensor results).  Each iteration synchronises once: the class model is host arithmetic on the K x 15
    sums.  Returns a ``_seg.SegResult``.  The defaults come from a sweep on one synthetic phantom.
    ``min_island`` > 0: the islands of the hard labels with fewer voxels take the class of their surroundings
    (``components.reassign_small``) and ``n_reassigned`` counts the voxels changed; 0 runs nothing new."""
    import torch

    require(*_abi.SEG_SYMBOLS)
    classes = _seg._classes(classes)
    if len(tuple(y.shape)) == 3:
        y = y[None]
    Cn, nz, ny, nx = _planes(y, "segment_em", "y")
    if tuple(prior.shape) != (len(classes), nz, ny, nx):
        raise ValueError(f"segment_em needs prior as (K, Z, Y, X) on y's grid, got {tuple(prior.shape)} for y {tuple(y.shape)}")
    _seg.check_em_arguments(len(classes), Cn, beta, prior_floor, var_floor, n_iter, tol)
    min_island = _seg.check_min_island(min_island)
    dev = pick_device((y, prior, mask), device)
    with torch.cuda.device(dev):
        yd = flat(y, dev).reshape(Cn, nz, ny, nx)
        M = effective_mask(yd, mask)
        pi = normalise_priors(flat(prior, dev).reshape(len(classes), nz, ny, nx), M, prior_floor)
        p, model, trace, it = _seg.run_em(pi, yd, M, Cn, DEVICE_STEPS, beta=beta, var_floor=var_floor, n_iter=n_iter, tol=tol)
        labels, changed = hard_labels(p, classes, M), 0
        if min_island:
            from ._gpu_components import reassign_small

            labels, changed = reassign_small(labels, min_island, device=dev.index)
    return _seg.SegResult(_host(labels, y), model, trace, it, _host(p, y) if return_posteriors else None, changed)
