"""Gibbs-ringing removal on the GPU (``t2map.unring``): local sub-voxel shifts (Kellner et al. 2016) on the matrix cores;
:mod:`fetal_t2mapping_amd._unring` states the result in numpy and builds the tables both paths read."""
import ctypes as C
import functools

import numpy as np

from . import _abi
from ._gpu import check_out, current_stream, is_tensor, pick_device, release, require, workspace
from ._lib import check, load
from ._unring import DEFAULT_K, DEFAULT_MAX_W, DEFAULT_MIN_W, Tables, check_params

AXES = {"x": 0, "y": 1, 0: 0, 1: 1}


@functools.lru_cache(maxsize=8)
def unring_tables(ny, nx, K=DEFAULT_K):
    """The :class:`_unring.Tables` of a slice size and shift count (float64 on the host, rounded once to float32); kept for the
    next call."""
    return Tables(ny, nx, K)


def tables_host(ny, nx, K=DEFAULT_K):
    """The packed tables (``uint8`` numpy array) as ``t2fit_unring_tables_host`` writes them, for C callers; no device."""
    lib = load()
    need = C.c_size_t(0)
    check(lib.t2fit_unring_tables_bytes(int(ny), int(nx), int(K), C.byref(need)))
    out = np.zeros(need.value, np.uint8)
    check(lib.t2fit_unring_tables_host(int(ny), int(nx), int(K), out.ctypes.data, out.nbytes))
    return out


def unring_params(K=DEFAULT_K, min_w=DEFAULT_MIN_W, max_w=DEFAULT_MAX_W):
    p = _abi.T2FitUnringParams()
    check(load().t2fit_unring_params_default(C.byref(p)))
    p.K, p.min_w, p.max_w = int(K), int(min_w), int(max_w)
    return p


def _tables_on(tables, dev):
    """The packed block of `tables` on `dev`; the Tables object keeps it for the next call."""
    import torch

    cache = tables.__dict__.setdefault("_packed_dev", {})
    key = str(dev)
    if key not in cache:
        t = torch.from_numpy(tables.pack()).to(dev)
        if t.data_ptr() % 16:
            raise RuntimeError("the device allocator returned a block that is not aligned to 16 bytes")
        cache[key] = t
    return cache[key]


def _slices(x, dev):
    """float32 (S, ny, nx), numpy array or tensor -> contiguous tensor on `dev`."""
    import torch

    t = x if is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))
    if t.dim() != 3:
        raise ValueError(f"unring takes slices (S, ny, nx), got shape {tuple(t.shape)}")
    if t.dtype != torch.float32:
        raise ValueError(f"unring takes float32 slices, got {t.dtype}")
    return t.to(dev).contiguous()


def _workspace(lib, params, s, ny, nx, dev):
    need = C.c_size_t(0)
    check(lib.t2fit_unring_workspace_bytes(C.byref(params), s, ny, nx, C.byref(need)))
    ws, ptr = workspace(need.value, dev)
    return ws, ptr, need.value


def unring_split(x, tables=None, device=0):
    """``(I1, I2)`` CUDA tensors (S, ny, nx): step 1, bit for bit :func:`_unring.split`.  I1 keeps the ringing along x, I2 the
    ringing along y."""
    import torch

    lib = require(*_abi.UNRING_SYMBOLS)
    dev = pick_device((x,), device)
    with torch.cuda.device(dev):
        t = _slices(x, dev)
        s, ny, nx = (int(v) for v in t.shape)
        tables = tables or unring_tables(ny, nx, DEFAULT_K)
        check_params(ny, nx, tables.K, 1, 1)
        params = unring_params(tables.K, 1, 1)
        blob = _tables_on(tables, dev)
        i1, i2 = torch.empty_like(t), torch.empty_like(t)
        ws, ptr, nbytes = _workspace(lib, params, s, ny, nx, dev)
        check(lib.t2fit_unring_split_dev(blob.data_ptr(), t.data_ptr(), s, ny, nx, i1.data_ptr(), i2.data_ptr(), ptr, nbytes, current_stream()))
        release(t, ws)
    return i1, i2


def unring_rows(x, axis="x", K=DEFAULT_K, min_w=DEFAULT_MIN_W, max_w=DEFAULT_MAX_W, tables=None, details=True, device=0):
    """Step 2 on the rows (``axis='x'``) or columns (``axis='y'``) of the slices x (S, ny, nx): ``(out, shift int8, tv float32)``
    CUDA tensors of x's shape (``details=False``: out alone; the library then gets NULL for the other two).  Bit for bit
    :func:`_unring.unring_rows`."""
    import torch

    if axis not in AXES:
        raise ValueError(f"axis must be 'x' or 'y', got {axis!r}")
    lib = require(*_abi.UNRING_SYMBOLS)
    dev = pick_device((x,), device)
    with torch.cuda.device(dev):
        t = _slices(x, dev)
        s, ny, nx = (int(v) for v in t.shape)
        n = nx if AXES[axis] == 0 else ny  # the limits hold along the rows; across them any size goes
        check_params(n, n, K, min_w, max_w)
        if tables is None:
            tables = unring_tables(ny, nx, int(K)) if min(ny, nx) >= _abi.UNRING_MIN_N else unring_tables(n, n, int(K))
        params = unring_params(K, min_w, max_w)
        blob = _tables_on(tables, dev)
        out = torch.empty_like(t)
        shift = torch.empty(t.shape, dtype=torch.int8, device=dev) if details else None
        tv = torch.empty_like(t) if details else None
        check(lib.t2fit_unring_rows_dev(C.byref(params), blob.data_ptr(), t.data_ptr(), s, ny, nx, AXES[axis], out.data_ptr(),
                                        shift.data_ptr() if details else None, tv.data_ptr() if details else None, current_stream()))
        release(t)
    return (out, shift, tv) if details else out


def unring_slices(x, K=DEFAULT_K, min_w=DEFAULT_MIN_W, max_w=DEFAULT_MAX_W, tables=None, details=False, out=None, device=0):
    """The whole stage on slices (S, ny, nx): ``(out, skipped)`` with out a CUDA tensor, or with ``details`` ``(out, skipped,
    shift int8 (2, S, ny, nx), tv float32 (2, S, ny, nx))`` (axis x first).  A slice with a non-finite sample is copied and
    counted in ``skipped``; a constant slice is copied.  Bit for bit :func:`_unring.unring`."""
    import torch

    lib = require(*_abi.UNRING_SYMBOLS)
    dev = pick_device((x, out), device)
    with torch.cuda.device(dev):
        t = _slices(x, dev)
        s, ny, nx = (int(v) for v in t.shape)
        check_params(ny, nx, K, min_w, max_w)
        tables = tables or unring_tables(ny, nx, int(K))
        params = unring_params(K, min_w, max_w)
        blob = _tables_on(tables, dev)
        if out is None:
            out = torch.empty_like(t)
        else:
            check_out(out, torch.float32, (s, ny, nx), dev)
            if out.data_ptr() == t.data_ptr():
                raise ValueError("out must not be the input")
        shift = torch.empty((2, s, ny, nx), dtype=torch.int8, device=dev) if details else None
        tv = torch.empty((2, s, ny, nx), dtype=torch.float32, device=dev) if details else None
        skipped = C.c_int64(0)
        ws, ptr, nbytes = _workspace(lib, params, s, ny, nx, dev)
        check(lib.t2fit_unring_dev(C.byref(params), blob.data_ptr(), t.data_ptr(), s, ny, nx, out.data_ptr(),
                                   shift.data_ptr() if details else None, tv.data_ptr() if details else None, C.byref(skipped), ptr, nbytes,
                                   current_stream()))
        release(t, ws)
    return (out, int(skipped.value), shift, tv) if details else (out, int(skipped.value))


def unring_volume(block, slice_axis=0, K=DEFAULT_K, min_w=DEFAULT_MIN_W, max_w=DEFAULT_MAX_W, out=None, info=None, device=0):
    """Unring every slice of a float32 block ``(..., Z, Y, X)`` of any leading shape.  ``slice_axis`` (0, 1 or 2) names, among the
    last three axes, the one the slices were acquired along: the other two span the plane that is filtered, and must be
    acquired voxels, not interpolated ones.  A numpy block gives a numpy block, a tensor a tensor; ``out`` (same kind, shape
    and dtype, not the input) receives the result; ``info``, a dict, receives ``skipped``."""
    import torch

    if slice_axis not in (0, 1, 2):
        raise ValueError(f"slice_axis must be 0, 1 or 2 (among the last three axes), got {slice_axis!r}")
    shape = tuple(int(v) for v in block.shape)
    if len(shape) < 3:
        raise ValueError(f"unring_volume takes a block (..., Z, Y, X), got shape {shape}")
    if (block.dtype != torch.float32) if is_tensor(block) else (np.asarray(block).dtype != np.float32):
        raise ValueError(f"unring_volume takes a float32 block, got {block.dtype}")
    dev = pick_device((block, out if is_tensor(out) else None), device)
    if out is not None:
        if is_tensor(block):
            check_out(out, torch.float32, shape, dev)
        else:
            check_out(out, "float32", shape, None)
    t = block if is_tensor(block) else torch.from_numpy(np.ascontiguousarray(block))
    t = t.to(dev)
    nd = t.dim()
    src = nd - 3 + slice_axis
    moved = t.movedim(src, nd - 3).contiguous()  # (..., slices, plane rows, plane columns)
    ny, nx = int(moved.shape[-2]), int(moved.shape[-1])
    res, skipped = unring_slices(moved.reshape(-1, ny, nx), K, min_w, max_w, device=device)
    res = res.reshape(moved.shape).movedim(nd - 3, src)
    if info is not None:
        info["skipped"] = skipped
    if is_tensor(block):
        if out is None:
            return res.contiguous()
        out.copy_(res)
        return out
    host = res.contiguous().cpu().numpy()
    if out is None:
        return host
    out[...] = host
    return out
