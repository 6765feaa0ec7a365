"""Connected components on the GPU (``t2map.components``): labels, sizes, boxes, centroid sums, island removal and seeds.
:mod:`fetal_t2mapping_amd._components` states every result in numpy; the device results equal it in every element, and
for a mask ``scipy.ndimage.label``."""
import ctypes as C

import numpy as np

from . import _abi, _components
from ._gpu import current_stream, int_labels, is_tensor, pick_device, release, require, volume, workspace
from ._lib import check

TILE = _abi.COMPONENTS_TILE  # (z, y, x) voxels of the tile a workgroup labels in LDS; results do not depend on it


def _is_mask(vol):
    """A uint8 or bool volume is a mask (foreground = not 0); any other integer dtype holds classes."""
    import torch

    if is_tensor(vol):
        return vol.dtype in (torch.uint8, torch.bool)
    dt = np.asarray(vol).dtype
    return dt == np.uint8 or dt == np.bool_


def _input(vol, dev):
    """``(tensor on dev, in_type)``: a mask as uint8, classes as int32."""
    import torch

    if _is_mask(vol):
        return volume(vol, torch.uint8, dev, "volume"), _abi.MORPH_U8
    t = int_labels(vol, dev)
    if t.dim() != 3:
        raise ValueError(f"volume must be 3-D (z, y, x), got shape {tuple(t.shape)}")
    if t.dtype != torch.int32:
        if bool(((t < -2**31) | (t >= 2**31)).any()):
            raise ValueError("classes must fit int32")
        t = t.to(torch.int32)
    return t.contiguous(), _abi.MORPH_I32


def _label_volume(labels, dev):
    import torch

    t = int_labels(labels, dev)
    if t.dim() != 3:
        raise ValueError(f"labels must be 3-D (z, y, x), got shape {tuple(t.shape)}")
    if t.dtype != torch.int32:  # values beyond int32 are outside every table
        t = torch.where((t >= 0) & (t < 2**31), t, torch.full_like(t, -1)).to(torch.int32)
    return t.contiguous()


def label(vol, connectivity=1, *, device=0):
    """``(labels, n)``: int32 CUDA tensor shaped like ``vol`` (z, y, x) -- 0 on the background, 1..n on the components,
    numbered by their first voxel as ``scipy.ndimage.label`` numbers them -- and the count.  ``vol``: a numpy array or
    tensor; uint8 / bool is a mask, any other integer dtype classes (connected = neighbours with the same value, not 0).
    ``connectivity`` 1, 2, 3: 6, 18, 26 neighbours.  The call waits for the current stream once, for the count."""
    import torch

    lib = require(*_abi.COMPONENT_SYMBOLS)
    if connectivity not in (1, 2, 3):
        raise ValueError(f"connectivity must be 1, 2 or 3, got {connectivity!r}")
    dev = pick_device((vol,), device)
    with torch.cuda.device(dev):
        t, in_type = _input(vol, dev)
        nz, ny, nx = (int(v) for v in t.shape)
        need = C.c_size_t(0)
        check(lib.t2fit_components_workspace_bytes(nz, ny, nx, C.byref(need)))
        ws, ptr = workspace(need.value, dev)
        out = torch.empty((nz, ny, nx), dtype=torch.int32, device=dev)
        n = C.c_int32(0)
        check(lib.t2fit_components_label_dev(t.data_ptr(), in_type, nz, ny, nx, int(connectivity), out.data_ptr(), C.byref(n), ptr,
                                             need.value, current_stream()))
        release(t, ws)
    return out, int(n.value)


def _tables(lab, n, want):
    """The tables named in `want` ("sizes", "bbox", "sums") of the int32 device volume `lab`, the others None: the library
    skips what it is not asked for."""
    import torch

    lib = require(*_abi.COMPONENT_SYMBOLS)
    dev = lab.device
    with torch.cuda.device(dev):
        sizes = torch.empty(n + 1, dtype=torch.int64, device=dev) if "sizes" in want else None
        bbox = torch.empty((n + 1, 6), dtype=torch.int32, device=dev) if "bbox" in want else None
        sums = torch.empty((n + 1, 3), dtype=torch.int64, device=dev) if "sums" in want else None
        check(lib.t2fit_components_stats_dev(lab.data_ptr(), lab.shape[0], lab.shape[1], lab.shape[2], n,
                                             *(None if t is None else t.data_ptr() for t in (sizes, bbox, sums)), current_stream()))
        release(lab)
    return sizes, bbox, sums


def stats(labels, n, *, device=0):
    """``(sizes int64 (n + 1,), bbox int32 (n + 1, 6), sums int64 (n + 1, 3))`` CUDA tensors of the values 0..n of an
    integer label volume (row 0: the background; other values are ignored): :func:`_components.stats`."""
    n = int(n)
    if n < 0:
        raise ValueError("n must not be negative")
    return _tables(_label_volume(labels, pick_device((labels,), device)), n, ("sizes", "bbox", "sums"))


def lut(sizes, *, min_size=0, max_size=0, largest=False, renumber=False, device=0):
    """``(table, n_kept)``: the selection table (int32 CUDA tensor, n + 1 entries) of :func:`_components.lut` from the
    device sizes of :func:`stats`, and the number kept (the call waits for the current stream once)."""
    import torch

    lib = require(*_abi.COMPONENT_SYMBOLS)
    _components.check_selection(min_size, max_size)
    dev = pick_device((sizes,), device)
    with torch.cuda.device(dev):
        s = (sizes if is_tensor(sizes) else torch.from_numpy(np.ascontiguousarray(sizes, np.int64))).to(dev, torch.int64).contiguous()
        if s.dim() != 1 or s.numel() < 1:
            raise ValueError("sizes must be a vector of n + 1 entries")
        table = torch.empty(s.numel(), dtype=torch.int32, device=dev)
        kept = C.c_int32(0)
        check(lib.t2fit_components_lut_dev(s.data_ptr(), s.numel() - 1, int(min_size), int(max_size), int(bool(largest)),
                                           int(bool(renumber)), table.data_ptr(), C.byref(kept), current_stream()))
        release(s)
    return table, int(kept.value)


def _relabel(lab, table):
    """``table[lab]`` through t2fit_relabel_dev, both on the device."""
    import torch

    lib = require(*_abi.MORPH_SYMBOLS)
    out = torch.empty_like(lab)
    with torch.cuda.device(lab.device):
        check(lib.t2fit_relabel_dev(lab.data_ptr(), lab.numel(), table.data_ptr(), table.numel(), out.data_ptr(), current_stream()))
        release(table)
    return out


def select(labels, n, *, min_size=0, max_size=0, largest=False, renumber=False, device=0):
    """The label volume with the components outside ``min_size..max_size`` (``max_size=0``: no upper limit) set to 0; with
    ``largest`` only the largest of the others stays (a tie: the lowest label); with ``renumber`` the kept are numbered
    1.. in label order.  int32 CUDA tensor; nothing but two counts leaves the device."""
    dev = pick_device((labels,), device)
    lab = _label_volume(labels, dev)
    sizes = _tables(lab, int(n), ("sizes",))[0]
    table, _ = lut(sizes, min_size=min_size, max_size=max_size, largest=largest, renumber=renumber, device=device)
    return _relabel(lab, table)


def keep_largest(mask, k=1, connectivity=1, *, device=0):
    """The ``k`` largest components of a mask as a uint8 CUDA tensor (ties: the lower label first).  ``k = 1`` runs
    entirely on the device.  ``k > 1`` reads the n sizes back and builds the table with a stable sort on the host."""
    import torch

    if int(k) < 1:
        raise ValueError("k must be at least 1")
    dev = pick_device((mask,), device)
    m = volume(mask, torch.uint8, dev, "mask")
    lab, n = label(m, connectivity, device=device)
    if int(k) == 1:
        return (select(lab, n, largest=True, device=device) != 0).to(torch.uint8)
    sizes = _tables(lab, n, ("sizes",))[0].cpu().numpy()
    table = torch.from_numpy(_components.largest_lut(sizes, k)).to(dev)
    return (_relabel(lab, table) != 0).to(torch.uint8)


def remove_small(vol, min_size, connectivity=1, *, device=0):
    """``vol`` without the components of fewer than ``min_size`` voxels.  A mask (uint8 / bool) gives a uint8 mask;
    integer classes give int32 classes with the small islands set to 0.  CUDA tensor."""
    import torch

    dev = pick_device((vol,), device)
    t, _ = _input(vol, dev)
    lab, n = label(t, connectivity, device=device)
    kept = select(lab, n, min_size=min_size, device=device) != 0
    return kept.to(torch.uint8) if _is_mask(vol) else torch.where(kept, t, torch.zeros_like(t))


def seeds(mask, connectivity=1, min_size=1, max_size=0, *, device=0):
    """The centroids of the mask's components whose size lies in ``min_size..max_size`` (0: no upper limit), rounded half
    up in integers, as a list of ``[x, y, z]`` in label order: what ``--phantom_seeds`` reads.  The sizes and sums of the
    kept components are read back; the rounding is host integer arithmetic."""
    import torch

    dev = pick_device((mask,), device)
    lab, n = label(volume(mask, torch.uint8, dev, "mask"), connectivity, device=device)
    sizes = _tables(lab, n, ("sizes",))[0]
    table, kept = lut(sizes, min_size=min_size, max_size=max_size, renumber=True, device=device)
    sizes, _, sums = _tables(_relabel(lab, table), kept, ("sizes", "sums"))
    return [[int(v) for v in row] for row in _components.centroids(sizes.cpu().numpy(), sums.cpu().numpy())]


def reassign_small(classes, min_size, connectivity=1, spacing=None, *, device=0):
    """``(classes, n_changed)``: every island of fewer than ``min_size`` voxels takes, voxel by voxel, the class at its
    nearest site -- the sites being the voxels that are not 0 and not in a small island -- instead of leaving a hole as
    :func:`remove_small` does (:func:`_edt.reassign_small`).  ``classes``: an integer volume (bool: a mask); ``spacing``:
    ``(sz, sy, sx)`` of the distance, default 1.  Class 0 stays 0; one round; with no site nothing changes.  A speck
    surrounded by class 0 takes a class but stays a speck: that is :func:`remove_small`'s job.  int32 CUDA tensor and the
    number of voxels changed (the call waits for the stream for the counts)."""
    import torch

    from . import _gpu_edt

    if int(min_size) < 0:
        raise ValueError("min_size must not be negative")
    dev = pick_device((classes,), device)
    if is_tensor(classes) and classes.dtype == torch.uint8:
        classes = classes.to(torch.int32)
    elif not is_tensor(classes) and np.asarray(classes).dtype == np.uint8:
        classes = np.asarray(classes).astype(np.int32)
    t, _ = _input(classes, dev)
    t = t.to(torch.int32)
    lab, n = label(t, connectivity, device=device)
    sizes = _tables(lab, n, ("sizes",))[0]
    table, _ = lut(sizes, min_size=int(min_size), device=device)
    kept = _relabel(lab, table) != 0
    small = (lab != 0) & ~kept
    index = _gpu_edt._nearest(kept, 0, spacing, dev, want_d2=False)[1]
    out = _gpu_edt.fill_nearest(t, small, index, device=device)
    return out, int((out != t).sum())
