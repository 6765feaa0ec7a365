"""Resampling and the orthogonal-stack reconstruction on the GPU; :mod:`fetal_t2mapping_amd._resample` states both
in numpy."""
import ctypes as C

import numpy as np

from . import _abi, _resample
from ._gpu import current_stream, flat, is_tensor, pick_device, release, require, workspace
from ._lib import check


_INT32_RANGE = (-2 ** 31, 2 ** 31 - 1)


def _labels_fit_int32(vol, is_t):
    """Refuse an integer volume whose ids do not fit the int32 the kernel copies (a cast would wrap them silently), with
    their range in the message.  Returns the volume to convert: itself, or for torch's unsigned 32- and 64-bit types
    (which torch neither reduces nor converts everywhere) the same bits as the signed type, equal in value once they
    fit.  A tensor is reduced once where it lives and two numbers are read back: one synchronisation for a CUDA tensor."""
    import torch

    if (vol.numel() if is_t else vol.size) == 0:
        return vol
    wrap = 0
    if not is_t:
        lo, hi = int(vol.min()), int(vol.max())
    else:
        if vol.dtype in (torch.uint32, torch.uint64):
            wrap = 2 ** (8 * vol.dtype.itemsize)
            vol = vol.contiguous().view(torch.int32 if vol.dtype == torch.uint32 else torch.int64)
        lo, hi = (int(v) for v in torch.stack(torch.aminmax(vol)).tolist())
        if wrap and lo < 0:  # negative as signed is the upper half as unsigned; the refusal may take its time
            neg, pos = vol[vol < 0], vol[vol >= 0]
            hi = int(neg.max()) + wrap
            lo = int(pos.min()) if pos.numel() else int(neg.min()) + wrap
    if lo < _INT32_RANGE[0] or hi > _INT32_RANGE[1]:
        raise ValueError(f"the label volume ({'u' if wrap else ''}{str(vol.dtype).split('.')[-1]}) holds values in [{lo}, {hi}], which do "
                         f"not fit int32 [{_INT32_RANGE[0]}, {_INT32_RANGE[1]}]: renumber the ids before resampling")
    return vol


def resample_volume(vol, geom, *, res=None, like=None, transform=None, interp="linear", default=0.0, integer_cast=False,
                    device=0):
    """Resample ``vol`` -- ``(Z, Y, X)`` or ``(n, Z, Y, X)`` volumes that share the geometry ``geom`` (anything with
    GetSpacing / GetOrigin / GetDirection: a ``nifti.Image``) -- on the GPU.  The output grid is ``geom`` at ``res`` mm
    isotropic (the reference's ``resample_volume``, utils/qmri_utils.py:62-80; the default with ``res=1.0``) or the grid
    ``like`` (anything with the four Get* methods including GetSize, e.g. a :class:`_resample.Geometry`).  ``transform``:
    4 x 4, maps a physical point of the output grid to a physical point of ``vol`` (``sitk.Resample``'s sense).
    ``interp='linear'`` takes float32 and returns float32; ``'nearest'`` copies float32 or int32 (label / mask volumes:
    any integer type whose values fit int32 comes back as int32, one whose values do not is refused with a ValueError
    that names their range).
    ``integer_cast``: truncate toward zero and clamp to int16's range, as a stack that keeps an int16 pixel type does.
    numpy in, numpy out; CUDA tensor in, tensor out (asynchronous on the current stream, except that an integer tensor
    wider than int32 -- int64, uint32, uint64 -- is first reduced to its range and that range read back: one
    synchronisation).  Returns ``(out, geometry)``.
    :mod:`fetal_t2mapping_amd._resample` states the definition in numpy; the result is bit-identical to it."""
    import torch

    is_t = is_tensor(vol)
    if not is_t:
        vol = np.asarray(vol)
    if is_t:  # the integer types torch has; bool and the floating types go through float32
        as_int = not (vol.dtype.is_floating_point or vol.dtype.is_complex or vol.dtype == torch.bool)
        wide = vol.dtype.itemsize > 4 or vol.dtype == torch.uint32
    else:
        as_int, wide = vol.dtype.kind in "iu", vol.dtype.itemsize > 4 or vol.dtype == np.uint32
    if as_int and wide:  # before the library is asked for: the refusal needs no device
        vol = _labels_fit_int32(vol, is_t)
    lib = require(*_abi.RECON_SYMBOLS)
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
    dev = pick_device((vol,), device)
    if as_int and interp != "nearest":
        raise ValueError("an integer volume is resampled with interp='nearest'")
    src = flat(vol, dev, dtype="int32" if as_int else "float32")
    oz, oy, ox = dst_geom.shape
    out = torch.empty((n_vol, oz, oy, ox) if len(shape) == 4 else (oz, oy, ox), dtype=src.dtype, device=dev)
    with torch.cuda.device(dev):
        check(lib.t2fit_resample_dev(src.data_ptr(), _abi.RESAMPLE_I32 if as_int else _abi.RESAMPLE_F32, *shape[-3:],
                                     A.ctypes.data_as(C.POINTER(C.c_double)), out.data_ptr(), oz, oy, ox, n_vol,
                                     _abi.INTERPS[interp], float(default), _abi.RESAMPLE_INTEGER_CAST if integer_cast else 0,
                                     current_stream()))
        release(src)
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

    from . import nifti

    lib = require(*_abi.RECON_SYMBOLS)
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
    dev = pick_device([stacks[o] for o in order], device)
    src = [flat(stacks[o], dev) for o in order]
    lo_size = (C.c_int32 * 9)(*[v for o in order for v in shapes[o][-3:]])
    hi_size = (C.c_int32 * 9)(*[v for g in hi for v in g.shape])
    A1 = (C.c_double * 36)(*np.concatenate([a.ravel() for a in a1]))
    A2 = (C.c_double * 24)(*np.concatenate([a.ravel() for a in a2]))
    flags = (_abi.RESAMPLE_INTEGER_CAST if integer_cast else 0) | (_abi.RECON_CHAIN if form == "chain" else 0)
    need = C.c_size_t(0)
    check(lib.t2fit_reconstruct_workspace_bytes(n_vol, lo_size, hi_size, flags, C.byref(need)))
    out = torch.empty((n_vol,) + hi[0].shape, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws, ws_ptr = workspace(need.value, dev) if need.value else (None, None)
        ptrs = (C.c_void_p * 3)(*[t.data_ptr() for t in src])
        check(lib.t2fit_reconstruct_dev(ptrs, lo_size, A1, hi_size, A2, out.data_ptr(), n_vol, flags, ws_ptr, need.value,
                                        current_stream()))
        release(ws, *src)
    g = hi[0]  # the grid as an image over an empty array: spacing / origin / direction for the writer
    return out, nifti.Image(np.zeros((0, 0, 0), np.float32), g.GetSpacing(), g.GetOrigin(), g.GetDirection())
