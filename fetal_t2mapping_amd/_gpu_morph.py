"""Masks and phantom labels on the GPU: binary morphology, hole filling, seed labels, and the reference's recipes built
from them (utils/qmri_utils.py build_mask :223-252, build_phantom_masks :591-623, build_phantom_labels_v2 :868-933,
build_mask_from_labels :935-951, convert_synthseg_to_feta :976-1009).  :mod:`fetal_t2mapping_amd._morph` states the
operations in numpy."""
import ctypes as C

import numpy as np

from . import _abi, _morph
from ._gpu import check_out, current_stream, int_labels, is_tensor, pick_device, release, require, volume, workspace
from ._lib import check


def _element(element):
    """(runs int32 (n, 4), size int32 (3,)) from a boolean footprint or a ``(runs, size)`` pair."""
    runs, size = _morph._as_runs(element)
    _morph._footprint(np.zeros(size, bool))  # odd sizes, radius <= 32: the message names the footprint
    return np.ascontiguousarray(runs, np.int32), np.asarray(size, np.int32)


def _morph_workspace(lib, shape, reach, dev):
    need = C.c_size_t(0)
    check(lib.t2fit_morph_workspace_bytes(shape[0], shape[1], shape[2], int(reach), C.byref(need)))
    ws, ptr = workspace(need.value, dev)
    return ws, ptr, need.value


def _mask_and_out(mask, out, device):
    """The mask as a uint8 volume on the GPU and the tensor the result goes to: `out` checked, or a new one."""
    import torch

    m = volume(mask, torch.uint8, pick_device((mask,), device), "mask")
    if out is None:
        return m, torch.empty_like(m)
    check_out(out, torch.uint8, m.shape, m.device)
    return m, out


def binary_threshold(vol, lo=-np.inf, hi=np.inf, *, device=0):
    """``lo <= vol <= hi`` as a uint8 (0 / 1) CUDA tensor shaped like ``vol``: a float32 or int32 numpy array or tensor
    (other dtypes are converted to float32, integer ones to int32).  The comparison is exact; a NaN gives 0."""
    import torch

    lib = require(*_abi.MORPH_SYMBOLS)
    t = vol if is_tensor(vol) else torch.from_numpy(np.ascontiguousarray(vol))
    integer = not t.dtype.is_floating_point
    dev = pick_device((t,), device)
    t = t.to(dev, torch.int32 if integer else torch.float32).contiguous()
    out = torch.empty(t.shape, dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.t2fit_binary_threshold_dev(t.data_ptr(), _abi.MORPH_I32 if integer else _abi.MORPH_F32, t.numel(), float(lo),
                                             float(hi), out.data_ptr(), current_stream()))
    return out


def _binary_morph(op, mask, element, iterations, border_value, unbounded, out, device):
    import torch

    lib = require(*_abi.MORPH_SYMBOLS)
    runs, size = _element(element)
    m, out = _mask_and_out(mask, out, device)
    reach = int(size.max() // 2) * int(iterations) if unbounded else 0
    with torch.cuda.device(m.device):
        ws, ptr, nbytes = _morph_workspace(lib, m.shape, reach, m.device)
        check(lib.t2fit_binary_morph_dev(_abi.MORPH_OPS[op], m.data_ptr(), out.data_ptr(), m.shape[0], m.shape[1], m.shape[2],
                                         size.ctypes.data, runs.ctypes.data, len(runs), int(iterations), int(border_value),
                                         _abi.MORPH_UNBOUNDED if unbounded else 0, ptr, nbytes, current_stream()))
        release(ws)
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

    lib = require(*_abi.MORPH_SYMBOLS)
    if slice_axis not in (None, 0, 1, 2):
        raise ValueError("slice_axis must be None, 0, 1 or 2")
    m, out = _mask_and_out(mask, out, device)
    sweeps = C.c_int32(0)
    with torch.cuda.device(m.device):
        ws, ptr, nbytes = _morph_workspace(lib, m.shape, 0, m.device)
        check(lib.t2fit_fill_holes_dev(m.data_ptr(), out.data_ptr(), m.shape[0], m.shape[1], m.shape[2],
                                       -1 if slice_axis is None else int(slice_axis), ptr, nbytes, C.byref(sweeps),
                                       current_stream()))
        release(ws)
    return (out, int(sweeps.value)) if return_sweeps else out


def seed_labels(shape, seeds, element, *, labels=None, dtype="uint8", device=0):
    """``out[v] = max over seeds s of labels[s] * [v - seed_s in element]`` as a CUDA tensor of ``shape`` (z, y, x).
    ``seeds``: ``(x, y, z)`` indices, as the reference indexes an image; ``labels`` default to 1..n; ``dtype``
    'uint8' or 'int32'.  What leaves the volume is clipped."""
    import torch

    lib = require(*_abi.MORPH_SYMBOLS)
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
                                        _abi.MORPH_U8 if dtype == "uint8" else _abi.MORPH_I32, ptr, nbytes, current_stream()))
        release(ws)
    return out


def relabel(labels, lut, *, device=0):
    """``lut[labels]`` where ``0 <= labels < len(lut)``, else 0: an int32 CUDA tensor shaped like ``labels``."""
    import torch

    lib = require(*_abi.MORPH_SYMBOLS)
    dev = pick_device((labels,), device)
    lab = int_labels(labels, dev)
    if lab.dtype != torch.int32:  # ids beyond int32 are outside every table
        lab = torch.where((lab >= 0) & (lab < 2**31), lab, torch.full_like(lab, -1)).to(torch.int32)
    lab = lab.contiguous()
    table = torch.from_numpy(np.ascontiguousarray(lut, np.int32)).to(dev)
    out = torch.empty_like(lab)
    with torch.cuda.device(dev):
        check(lib.t2fit_relabel_dev(lab.data_ptr(), lab.numel(), table.data_ptr(), table.numel(), out.data_ptr(),
                                    current_stream()))
        release(table)
    return out


def _above(threshold):
    """The smallest float32 strictly above `threshold`: ``v > threshold`` for a float32 v is ``v >= _above(threshold)``."""
    f = np.float32(threshold)
    return float(f) if float(f) > float(threshold) else float(np.nextafter(f, np.float32(np.inf)))


def _clean(m, keep_largest, min_size, connectivity, device):
    """The island removal of build_mask / phantom_mask on the 3-D result; with the defaults the mask itself, untouched."""
    keep_largest, min_size = int(keep_largest), int(min_size)
    if keep_largest < 0 or min_size < 0:
        raise ValueError("keep_largest and min_size must not be negative")
    if not keep_largest and not min_size:
        return m
    from . import _gpu_components

    if min_size:
        m = _gpu_components.remove_small(m, min_size, connectivity, device=device)
    if keep_largest:
        m = _gpu_components.keep_largest(m, keep_largest, connectivity, device=device)
    return m


def build_mask(vol, threshold=1.0, slice_axis=2, size=5, *, device=0, keep_largest=0, min_size=0, connectivity=1):
    """The reference's ``build_mask``: ``vol > threshold``, then per plane perpendicular to ``slice_axis`` of the
    (z, y, x) array: fill holes, dilate and erode with a ``size x size`` square (scipy's borders).  uint8 CUDA tensor.
    Not the reference's: ``min_size`` > 0 drops the 3-D components (``connectivity`` 1, 2, 3) of fewer voxels from the
    result, ``keep_largest`` = k > 0 keeps its k largest (``t2map.components``); with the defaults neither runs."""
    if size < 1 or size % 2 == 0:
        raise ValueError("size must be odd")
    fp_shape = [size, size, size]
    fp_shape[slice_axis] = 1
    square = np.ones(fp_shape, bool)
    m = binary_threshold(np.asarray(vol, np.float32) if not is_tensor(vol) else vol.float(), _above(threshold), device=device)
    m = fill_holes(m, slice_axis=slice_axis, out=m)
    m = binary_dilate(m, square, out=m)
    return _clean(binary_erode(m, square, out=m), keep_largest, min_size, connectivity, device)


def phantom_mask(vol, threshold=100, close_radius=15, dilate_radius=10, *, device=0, keep_largest=0, min_size=0, connectivity=1):
    """The reference's ``build_phantom_masks`` for one echo volume: ``vol >= threshold``, 3-D fill holes, closing with
    the radius-``close_radius`` ball on the unbounded domain, dilation with the radius-``dilate_radius`` ball
    (:func:`_morph.ball`).  uint8 CUDA tensor.  ``keep_largest``, ``min_size``, ``connectivity``: as in
    :func:`build_mask`, off by default."""
    m = binary_threshold(np.asarray(vol, np.float32) if not is_tensor(vol) else vol.float(), float(threshold), device=device)
    m = fill_holes(m, out=m)
    m = binary_close(m, _morph.ball(close_radius), unbounded=True, out=m)
    return _clean(binary_dilate(m, _morph.ball(dilate_radius), out=m), keep_largest, min_size, connectivity, device)


def phantom_labels(shape, seeds, radius=6, *, device=0):
    """The reference's ``build_phantom_labels_v2``: a radius-``radius`` ball at every ``(x, y, z)`` seed carrying the
    seed's 1-based number, merged with a maximum.  uint8 CUDA tensor of ``shape`` (z, y, x)."""
    return seed_labels(shape, seeds, _morph.ball(radius), device=device)


def mask_from_labels(labels, *, device=0):
    """The reference's ``build_mask_from_labels``: ``labels >= 1`` as a uint8 CUDA tensor."""
    import torch

    lab = int_labels(labels, pick_device((labels,), device))
    # the sign is all that matters; int64 ids stay in range
    return binary_threshold(lab.clamp(min=-1, max=1).to(torch.int32), 1, device=device)


def synthseg_to_feta(labels, *, device=0):
    """The reference's ``convert_synthseg_to_feta``: SynthSeg ids -> FeTA tissue classes 1..7, everything else 0
    (``_morph.SYNTHSEG_TO_FETA``).  int32 CUDA tensor."""
    return relabel(labels, _morph.feta_lut(), device=device)
