"""The exact Euclidean distance transform on the GPU (``t2map.distance``): squared distances, nearest sites, and what is
built from them -- nearest-site fills, Euclidean balls in millimetres of any radius, surfaces and surface distances.
:mod:`fetal_t2mapping_amd._edt` states every result in numpy; ``d2`` and ``index`` equal it in every bit, and ``sqrt(d2)``
equals ``scipy.ndimage.distance_transform_edt``.  A numpy array in gives numpy results, a tensor in CUDA tensors."""
import ctypes as C

import numpy as np

from . import _abi, _edt, _morph
from ._gpu import current_stream, int_labels, is_tensor, pick_device, release, require, volume, workspace
from ._lib import check

MAX_AXIS = _abi.EDT_MAX_AXIS


def _host(t, like):
    return t if is_tensor(like) else t.cpu().numpy()


def _spacing(spacing):
    s = _edt.check_spacing(spacing)
    return s, s.ctypes.data_as(C.POINTER(C.c_double))


def _nearest(vol, invert, spacing, dev, want_d2=True, want_index=True):
    """``(d2, index)`` CUDA tensors (None where not wanted) of a volume already on `dev`; any dtype, 0 / not 0."""
    import torch

    lib = require(*_abi.EDT_SYMBOLS)
    if invert not in (0, 1, False, True):
        raise ValueError(f"invert must be 0 or 1, got {invert!r}")
    s, s_ptr = _spacing(spacing)
    with torch.cuda.device(dev):
        m = volume(vol, torch.uint8, dev, "volume")
        nz, ny, nx = (int(v) for v in m.shape)
        need = C.c_size_t(0)
        check(lib.t2fit_edt_workspace_bytes(nz, ny, nx, C.byref(need)))
        ws, ptr = workspace(need.value, dev)
        d2 = torch.empty((nz, ny, nx), dtype=torch.float64, device=dev) if want_d2 else None
        index = torch.empty((nz, ny, nx), dtype=torch.int32, device=dev) if want_index else None
        check(lib.t2fit_edt_dev(m.data_ptr(), int(bool(invert)), nz, ny, nx, s_ptr, None if d2 is None else d2.data_ptr(),
                                None if index is None else index.data_ptr(), ptr, need.value, current_stream()))
        release(m, ws)
    return d2, index


def nearest(vol, invert=False, spacing=None, *, device=0):
    """``(d2, index)``: float64 squared distance from every voxel of ``vol`` (z, y, x) to the nearest site and int32 linear
    index of that site, the lowest among equally near ones (:func:`_edt.nearest`).  Sites: the voxels that are not 0, with
    ``invert`` the voxels that are 0.  ``spacing``: ``(sz, sy, sx)``, default 1.  With no site ``inf`` and ``-1``."""
    dev = pick_device((vol,), device)
    d2, index = _nearest(vol, invert, spacing, dev)
    return _host(d2, vol), _host(index, vol)


def edt(mask, spacing=None, *, squared=False, return_indices=False, device=0):
    """``scipy.ndimage.distance_transform_edt(mask, sampling=spacing)``: the distance to the nearest voxel that is 0
    (``inf`` if there is none), float64; ``squared``: its square, exact for unit and dyadic spacing.  With
    ``return_indices`` also the int32 LINEAR index of that voxel, ``(d, index)`` -- at ties the lowest index, which is
    not scipy's choice."""
    import torch

    dev = pick_device((mask,), device)
    d2, index = _nearest(mask, 1, spacing, dev, want_index=return_indices)
    d = d2 if squared else torch.sqrt(d2)
    return (_host(d, mask), _host(index, mask)) if return_indices else _host(d, mask)


def fill_nearest(labels, where, index, *, device=0):
    """``out[v] = labels[index[v]]`` where ``where[v] != 0`` and ``index[v] >= 0``, else ``labels[v]``: int32, shaped like
    ``labels`` (any integer dtype that fits int32)."""
    import torch

    lib = require(*_abi.EDT_SYMBOLS)
    dev = pick_device((labels, where, index), device)
    with torch.cuda.device(dev):
        lab = int_labels(labels, dev)
        if lab.dtype != torch.int32:
            if bool(((lab < -2**31) | (lab >= 2**31)).any()):
                raise ValueError("labels must fit int32")
            lab = lab.to(torch.int32)
        lab = lab.contiguous()
        w = where if is_tensor(where) else torch.from_numpy(np.ascontiguousarray(where))
        w = (w != 0).to(dev, torch.uint8).contiguous()
        idx = int_labels(index, dev).to(torch.int32).contiguous()
        if w.numel() != lab.numel() or idx.numel() != lab.numel() or lab.numel() < 1:
            raise ValueError("labels, where and index must have the same number of elements, at least 1")
        out = torch.empty_like(lab)
        check(lib.t2fit_edt_fill_dev(lab.data_ptr(), w.data_ptr(), idx.data_ptr(), lab.numel(), out.data_ptr(), current_stream()))
        release(lab, w, idx)
    return _host(out, labels)


def dilate_mm(mask, r, spacing=None, *, device=0):
    """The mask grown by a Euclidean ball of radius ``r`` in the units of ``spacing`` (:func:`_edt.dilate_mm`): uint8.
    Any radius, at a cost that does not depend on it; ``dilate_mm(m, r + 0.5)`` equals ``binary_dilate(m, ball(r))``."""
    import torch

    dev = pick_device((mask,), device)
    d2 = _nearest(mask, 0, spacing, dev, want_index=False)[0]
    return _host((d2 <= float(np.float64(r) ** 2)).to(torch.uint8), mask)


def erode_mm(mask, r, spacing=None, *, device=0):
    """The mask shrunk by that ball (:func:`_edt.erode_mm`): uint8.  The outside of the grid holds no site."""
    import torch

    dev = pick_device((mask,), device)
    d2 = _nearest(mask, 1, spacing, dev, want_index=False)[0]
    return _host((d2 > float(np.float64(r) ** 2)).to(torch.uint8), mask)


def _surface(mask, dev):
    import torch

    from ._gpu_morph import binary_erode

    m = volume(mask, torch.uint8, dev, "mask")
    return m & (binary_erode(m, _morph.cross(1), border_value=0, device=dev.index) == 0).to(torch.uint8)


def surface(mask, *, device=0):
    """The mask's voxels with a 6-neighbour outside it, the outside of the grid included (:func:`_edt.surface`): uint8."""
    return _host(_surface(mask, pick_device((mask,), device)), mask)


def surface_distances(a, b, spacing=None, *, device=0):
    """``hausdorff``, ``hd95``, ``assd``, ``n_a``, ``n_b`` of two masks (:func:`_edt.surface_distances`), a dict.  The
    two distance transforms and the gathers run on the device; the reductions are ``_edt.surface_reduce`` on the host
    over the gathered values."""
    import torch

    dev = pick_device((a, b), device)
    sa, sb = _surface(a, dev), _surface(b, dev)
    if sa.shape != sb.shape:
        raise ValueError("the two masks must share a grid")
    if not bool(sa.any()) or not bool(sb.any()):
        raise ValueError("surface_distances: a mask is empty, it has no surface")
    to_b = torch.sqrt(_nearest(sb, 0, spacing, dev, want_index=False)[0])
    to_a = torch.sqrt(_nearest(sa, 0, spacing, dev, want_index=False)[0])
    return _edt.surface_reduce(to_b[sa != 0].cpu().numpy(), to_a[sb != 0].cpu().numpy())
