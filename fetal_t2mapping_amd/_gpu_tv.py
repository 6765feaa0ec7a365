"""TV-Chambolle denoising of the echo stack on the GPU; :mod:`fetal_t2mapping_amd._tv` states the loop in numpy."""
import ctypes as C

from . import _abi
from ._gpu import check_out, current_stream, flat, is_tensor, pick_device, release, require, workspace
from ._lib import check


def tv_params(weight=0.1, eps=2e-4, max_iter=200, dims=2, precision="f32"):
    """The POD of :func:`denoise_tv` (``t2fit_tv_params``); the library checks the values."""
    if precision not in _abi.PRECISIONS:
        raise ValueError(f"precision must be 'f32' or 'f64', got {precision!r}")
    return _abi.T2FitTvParams(float(weight), float(eps), int(max_iter), int(dims), _abi.PRECISIONS[precision], 0)


def denoise_tv(echoes, weight=0.1, *, eps=2e-4, max_iter=200, dims=2, precision="f32", out=None, return_info=False,
               layout="te_major", device=0, max_workspace_bytes=None, joint=False):
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
    :mod:`fetal_t2mapping_amd._tv` states the same loop in numpy.

    ``joint=True``: vector-valued TV across the echoes (``t2fit_tv_joint_denoise_dev``, :func:`_tv.denoise_tv_joint`).  The
    stack must be ``(C, Z, Y, X)`` with at most ``_abi.TV_JOINT_MAX_CHAN`` channels; a problem is slice z of all echoes
    (``dims=2``: Z problems) or the whole stack (``dims=3``: one), and all echoes share one gradient norm per voxel, hence
    one edge set.  The weight is not rescaled by C: the joint norm of pure noise is about ``sqrt(C)`` times one echo's,
    so a weight that suits ``joint=False`` is about ``sqrt(C)`` too small.  A joint problem is never split across echoes:
    under ``max_workspace_bytes`` the slices are run in groups for ``dims=2`` (through a contiguous copy of each
    group), and ``dims=3`` is refused when the whole does not fit."""
    import torch

    lib = require(*(_abi.TV_SYMBOLS + (_abi.TVJ_SYMBOLS if joint else ())))
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
    is_t = is_tensor(echoes)
    if out is not None and not is_t:
        raise ValueError("out= goes with a CUDA tensor input (a numpy input returns a new array)")
    if joint:
        if len(shape) != 4:
            raise ValueError(f"denoise_tv(joint=True) needs a (C, Z, Y, X) stack of echoes, got shape {shape}")
        return _denoise_tv_joint(lib, echoes, par, shape, is_t, out, return_info, device, max_workspace_bytes)
    need = C.c_size_t(0)
    check(lib.t2fit_tv_workspace_bytes(C.byref(par), n_vol, nz, ny, nx, C.byref(need)))
    dev = pick_device((echoes,), device)
    src = flat(echoes, dev)
    if out is None:
        dst = torch.empty_like(src)
    else:
        check_out(out, torch.float32, shape, src.device)
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
        ws, ws_ptr = workspace(need.value, dev)
        stream = current_stream()
        n_v = nz * ny * nx
        for v0 in range(0, n_vol, group):
            g = min(group, n_vol - v0)
            check(lib.t2fit_tv_denoise_dev(C.byref(par), src.data_ptr() + 4 * v0 * n_v, dst.data_ptr() + 4 * v0 * n_v, g, nz,
                                           ny, nx, ws_ptr, need.value, n_iter.data_ptr() + 4 * v0 * n_prob_vol,
                                           energy.data_ptr() + 8 * v0 * n_prob_vol, stream))
        release(ws)
    host = (lambda t: t) if is_t else (lambda t: t.cpu().numpy())
    res = host(dst.reshape(shape))
    return (res, {"n_iter": host(n_iter), "energy": host(energy)}) if return_info else res


def _denoise_tv_joint(lib, echoes, par, shape, is_t, out, return_info, device, max_workspace_bytes):
    """The ``joint=True`` half of :func:`denoise_tv`."""
    import torch

    n_chan, nz, ny, nx = shape
    need = C.c_size_t(0)
    check(lib.t2fit_tv_joint_workspace_bytes(C.byref(par), n_chan, nz, ny, nx, C.byref(need)))
    dev = pick_device((echoes,), device)
    src = flat(echoes, dev)
    if out is None:
        dst = torch.empty_like(src)
    else:
        check_out(out, torch.float32, shape, src.device)
        dst = out.reshape(-1)
    n_prob = nz if par.dims == 2 else 1
    n_iter = torch.empty(n_prob, dtype=torch.int32, device=dev)
    energy = torch.empty(n_prob, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        budget = int(torch.cuda.mem_get_info(dev)[0] * 0.9) if max_workspace_bytes is None else int(max_workspace_bytes)
        group = nz
        if par.dims == 2:
            while group > 1 and need.value > budget:
                group = (group + 1) // 2
                check(lib.t2fit_tv_joint_workspace_bytes(C.byref(par), n_chan, group, ny, nx, C.byref(need)))
        elif need.value > budget:
            raise ValueError(f"denoise_tv(joint=True, dims=3): the workspace of the one problem, {need.value} bytes, does not fit "
                             f"into {budget} bytes, and a joint problem cannot be split across echoes (dims=2 runs slice by "
                             "slice)")
        ws, ws_ptr = workspace(need.value, dev)
        stream = current_stream()
        if group == nz:
            check(lib.t2fit_tv_joint_denoise_dev(C.byref(par), src.data_ptr(), dst.data_ptr(), n_chan, nz, ny, nx, ws_ptr,
                                                 need.value, n_iter.data_ptr(), energy.data_ptr(), stream))
        else:
            src4, dst4 = src.reshape(shape), dst.reshape(shape)
            for z0 in range(0, nz, group):
                g = min(group, nz - z0)
                slab = src4[:, z0:z0 + g].contiguous()  # the call takes one channel stride: nz * ny * nx of its own stack
                check(lib.t2fit_tv_joint_denoise_dev(C.byref(par), slab.data_ptr(), slab.data_ptr(), n_chan, g, ny, nx, ws_ptr,
                                                     need.value, n_iter.data_ptr() + 4 * z0, energy.data_ptr() + 8 * z0, stream))
                dst4[:, z0:z0 + g] = slab
        release(ws)
    host = (lambda t: t) if is_t else (lambda t: t.cpu().numpy())
    res = host(dst.reshape(shape))
    return (res, {"n_iter": host(n_iter), "energy": host(energy)}) if return_info else res
