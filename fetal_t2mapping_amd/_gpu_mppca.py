"""Marchenko-Pastur PCA denoising and noise maps across the echoes on the GPU; :mod:`fetal_t2mapping_amd._mppca` states
every step in numpy."""
import ctypes as C

from . import _abi
from ._gpu import check_out, current_stream, flat, is_tensor, mask_u8, pick_device, release, require, workspace
from ._lib import check


def mppca_params(radius=2, dims=2, estimator=2):
    """The POD of :func:`denoise_mppca` (``t2fit_mppca_params``); the library checks the values."""
    return _abi.T2FitMppcaParams(int(radius), int(dims), int(estimator), 0)


def _stack_shape(echoes, who):
    shape = tuple(int(v) for v in echoes.shape)
    if len(shape) != 4:
        raise ValueError(f"{who} needs a te-major (nTE, Z, Y, X) stack of echoes, got shape {shape}")
    return shape


def denoise_mppca(echoes, *, radius=2, dims=2, estimator=2, mask=None, out=None, return_maps=False, device=0,
                  max_workspace_bytes=None):
    """Marchenko-Pastur PCA denoising of the echo stack on the GPU (Veraart et al., NeuroImage 2016; MRtrix's
    ``dwidenoise``): a denoiser with no weight to tune.  Over a window of ``(2 radius + 1)^dims`` voxels the echoes form a
    matrix of low rank plus noise; the noise eigenvalues follow the Marchenko-Pastur law, which gives the noise level and
    the rank cut-off, and every voxel's decay is projected onto the signal subspaces of the windows that hold it.

    ``echoes``: float32 ``(nTE, Z, Y, X)`` with 2 .. ``_abi.MPPCA_MAX_TE`` echoes, numpy array (numpy results) or CUDA tensor
    (tensor results, asynchronous on the current stream).  ``dims=2``: the window spans x, y (every slice on its own),
    ``dims=3``: x, y, z.  ``radius``: 1 .. 4; the window must hold more voxels than there are echoes.  ``estimator``: 2
    (default) or 1, ``dwidenoise``'s two forms of the Marchenko-Pastur ratio.  ``mask``: ``(Z, Y, X)``, 0 / not 0; only
    windows centred inside it are decomposed (a voxel that no such window holds keeps its samples).  ``out``: a float32
    CUDA tensor of the stack's shape to write into (may be ``echoes`` itself); tensor input only.  ``return_maps``: also
    return ``{'sigma': float32 (Z, Y, X), 'rank': uint8 (Z, Y, X)}``, the noise level and the number of kept components of
    the window centred nearest to every voxel (0 where that window was not decomposed).  The noise is treated as Gaussian:
    at low SNR the Rician floor of magnitude data biases sigma low.

    The workspace (the projector of every window, ``8 nTE (nTE + 1) / 2`` bytes per voxel) is a torch buffer; when it would
    not fit into the free device memory (or ``max_workspace_bytes``) the slices are run in groups (``dims=2``) or in slabs
    with their halo of ``2 radius`` slices (``dims=3``), which changes no byte of any result.
    :mod:`fetal_t2mapping_amd._mppca` states the same computation in numpy; the device equals it bit for bit."""
    import torch

    lib = require(*_abi.MPPCA_SYMBOLS)
    shape = _stack_shape(echoes, "denoise_mppca")
    m, nz, ny, nx = shape
    par = mppca_params(radius, dims, estimator)
    is_t = is_tensor(echoes)
    if out is not None and not is_t:
        raise ValueError("out= goes with a CUDA tensor input (a numpy input returns a new array)")
    need = C.c_size_t(0)
    check(lib.t2fit_mppca_workspace_bytes(C.byref(par), m, nz, ny, nx, C.byref(need)))
    dev = pick_device((echoes,), device)
    src = flat(echoes, dev)
    n_v = nz * ny * nx
    msk = None if mask is None else mask_u8(mask, dev, n_v)
    if out is None:
        dst = torch.empty_like(src)
    else:
        check_out(out, torch.float32, shape, src.device)
        dst = out.reshape(-1)
    sigma = torch.empty(n_v, dtype=torch.float32, device=dev) if return_maps else None
    rank = torch.empty(n_v, dtype=torch.uint8, device=dev) if return_maps else None
    ptr = lambda t: None if t is None else t.data_ptr()
    halo = 2 * par.radius if par.dims == 3 else 0
    with torch.cuda.device(dev):
        budget = int(torch.cuda.mem_get_info(dev)[0] * 0.9) if max_workspace_bytes is None else int(max_workspace_bytes)
        group = nz
        while group > 1 and need.value > budget:
            group = (group + 1) // 2
            check(lib.t2fit_mppca_workspace_bytes(C.byref(par), m, min(nz, group + 2 * halo), ny, nx, C.byref(need)))
        if need.value > budget:
            raise ValueError(f"denoise_mppca: the workspace of one slice{' with its halo' if halo else ''}, {need.value} bytes, "
                             f"does not fit into {budget} bytes")
        ws, ws_ptr = workspace(need.value, dev)
        stream = current_stream()
        if group == nz:
            check(lib.t2fit_mppca_dev(C.byref(par), src.data_ptr(), ptr(msk), dst.data_ptr(), ptr(sigma), ptr(rank), m, nz, ny, nx,
                                      ws_ptr, need.value, stream))
        else:
            if halo and dst.data_ptr() == src.data_ptr():
                src = src.clone()  # a later slab reads the halo an earlier one has written
            src4, dst4 = src.reshape(shape), dst.reshape(shape)
            vol = (nz, ny, nx)
            for z0 in range(0, nz, group):
                z1 = min(z0 + group, nz)
                a, b = max(0, z0 - halo), min(nz, z1 + halo)
                slab = src4[:, a:b].contiguous()  # the call takes one echo stride: that of its own stack
                m_slab = None if msk is None else msk.reshape(vol)[a:b].contiguous()
                s_slab = None if sigma is None else torch.empty((b - a, ny, nx), dtype=torch.float32, device=dev)
                r_slab = None if rank is None else torch.empty((b - a, ny, nx), dtype=torch.uint8, device=dev)
                check(lib.t2fit_mppca_dev(C.byref(par), slab.data_ptr(), ptr(m_slab), slab.data_ptr(), ptr(s_slab), ptr(r_slab), m,
                                          b - a, ny, nx, ws_ptr, need.value, stream))
                dst4[:, z0:z1] = slab[:, z0 - a:z1 - a]
                if return_maps:
                    sigma.reshape(vol)[z0:z1] = s_slab[z0 - a:z1 - a]
                    rank.reshape(vol)[z0:z1] = r_slab[z0 - a:z1 - a]
                release(slab, m_slab, s_slab, r_slab)
        release(ws, msk)
    host = (lambda t: t) if is_t else (lambda t: t.cpu().numpy())
    res = host(dst.reshape(shape))
    if return_maps:
        return res, {"sigma": host(sigma.reshape(nz, ny, nx)), "rank": host(rank.reshape(nz, ny, nx))}
    return res


def mppca_noise_map(echoes, *, radius=2, dims=2, estimator=2, mask=None, device=0):
    """The noise map of :func:`denoise_mppca` alone: ``(sigma float32 (Z, Y, X), rank uint8 (Z, Y, X))`` of the echoes as
    they are, measured in tissue.  One kernel, no projector field and no workspace (``t2fit_mppca_dev`` with ``out_dev``
    NULL).  Arguments as in :func:`denoise_mppca`."""
    import torch

    lib = require(*_abi.MPPCA_SYMBOLS)
    m, nz, ny, nx = _stack_shape(echoes, "mppca_noise_map")
    par = mppca_params(radius, dims, estimator)
    need = C.c_size_t(0)
    check(lib.t2fit_mppca_workspace_bytes(C.byref(par), m, nz, ny, nx, C.byref(need)))  # (the refusals, before any copy)
    dev = pick_device((echoes,), device)
    src = flat(echoes, dev)
    n_v = nz * ny * nx
    msk = None if mask is None else mask_u8(mask, dev, n_v)
    sigma = torch.empty(n_v, dtype=torch.float32, device=dev)
    rank = torch.empty(n_v, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.t2fit_mppca_dev(C.byref(par), src.data_ptr(), None if msk is None else msk.data_ptr(), None, sigma.data_ptr(),
                                  rank.data_ptr(), m, nz, ny, nx, None, 0, current_stream()))
        release(src, msk)
    host = (lambda t: t) if is_tensor(echoes) else (lambda t: t.cpu().numpy())
    return host(sigma.reshape(nz, ny, nx)), host(rank.reshape(nz, ny, nx))
