"""Non-rigid alignment (a B-spline free-form deformation under Mattes mutual information) with the per-voxel steps on
the GPU; :mod:`fetal_t2mapping_amd._ffd` states the steps in numpy and holds the metric arithmetic, the regulariser and
the loop, which run here unchanged."""
import ctypes as C

import numpy as np

from . import _abi, _ffd, _register, _resample
from ._gpu import current_stream, is_tensor, pick_device, release, require, volume, workspace
from ._gpu_morph import build_mask
from ._gpu_register import DeviceAffinePyramid, _bins_tensor, _ones_like
from ._lib import check


def workspace_bytes(shape, side):
    """What t2fit_ffd_workspace_bytes returns for a fixed grid of ``shape`` (Z, Y, X): the axis tables, the gradient's row
    sums ``[rows][3][c]`` and plane sums ``[nz][3][c][c]``, a minimum and a count per row; each rounded up to 256 bytes."""
    nz, ny, nx = (int(v) for v in shape)
    side, rows, n_axis = int(side), nz * ny, nz + ny + nx
    parts = (4 * n_axis, 64 * n_axis, 8 * rows * 3 * side, 8 * nz * 3 * side * side, 8 * rows, 8 * rows)
    return sum((p + 255) // 256 * 256 for p in parts)


def _a12(A):
    return np.ascontiguousarray(A, np.float64).reshape(12)


class DeviceFFDPyramid(DeviceAffinePyramid):
    """:class:`_gpu_register.DeviceAffinePyramid` and the four steps of :class:`_ffd.HostFFDPyramid`.  ``hist`` and
    ``gradient`` upload the lattice (and the table) and copy their result back, which waits for the stream: the host makes
    the metric, the table and the next lattice in between."""

    def __init__(self, fixed, fixed_mask, moving, moving_mask, dev):
        super().__init__(fixed, fixed_mask, moving, moving_mask, dev)
        self.lib = require(*(_abi.REGISTER_SYMBOLS + _abi.ATLAS_SYMBOLS + _abi.FFD_SYMBOLS))
        self._ffd_bufs = {}

    def _lattice(self, phi, side=None):
        import torch

        phi = _ffd.check_lattice(phi, side)
        return torch.from_numpy(phi).to(self.dev), phi.shape[1]  # (pageable memory: the copy has left the host when it returns)

    def _workspace(self, shape, side):
        key = (tuple(int(v) for v in shape), int(side))
        if key not in self._ffd_bufs:
            need = C.c_size_t(0)
            check(self.lib.t2fit_ffd_workspace_bytes(*key[0], key[1], C.byref(need)))
            self._ffd_bufs = {key: workspace(need.value, self.dev) + (need.value,)}
        return self._ffd_bufs[key]

    def hist(self, level, bins, n_f, n_m, lo_m, scale_m, A, phi):
        import torch

        _, fmask, moving, mmask = level[:4]
        n_f, n_m = _register._check_bins(n_f), _register._check_moving_bins(n_m)
        a = _a12(A)
        with torch.cuda.device(self.dev):
            lat, side = self._lattice(phi)
            _, ptr, nbytes = self._workspace(fmask.shape, side)
            out = torch.empty(n_f * n_m, dtype=torch.int64, device=self.dev)
            check(self.lib.t2fit_ffd_joint_hist_dev(
                bins.data_ptr(), fmask.data_ptr(), *fmask.shape, moving.data_ptr(), mmask.data_ptr(), *moving.shape,
                a.ctypes.data_as(C.POINTER(C.c_double)), lat.data_ptr(), side, n_f, n_m, float(lo_m), float(scale_m), out.data_ptr(), ptr,
                nbytes, current_stream()))
            return out.cpu().numpy().view(np.uint64).reshape(n_f, n_m)  # (waits)

    def gradient(self, level, bins, table, n_m, lo_m, scale_m, A, phi):
        import torch

        _, fmask, moving, mmask = level[:4]
        table = np.ascontiguousarray(table, np.float64)
        if table.ndim != 2 or table.shape[1] != int(n_m):
            raise ValueError("table is float64 (n_f, n_m)")
        n_f, n_m = _register._check_bins(table.shape[0]), _register._check_moving_bins(n_m)
        a = _a12(A)
        with torch.cuda.device(self.dev):
            lat, side = self._lattice(phi)
            _, ptr, nbytes = self._workspace(fmask.shape, side)
            table_dev = torch.from_numpy(table.ravel()).to(self.dev)
            out = torch.empty((3, side, side, side), dtype=torch.float64, device=self.dev)
            check(self.lib.t2fit_ffd_gradient_dev(
                bins.data_ptr(), table_dev.data_ptr(), n_f, n_m, float(lo_m), float(scale_m), fmask.data_ptr(), *fmask.shape,
                moving.data_ptr(), mmask.data_ptr(), *moving.shape, a.ctypes.data_as(C.POINTER(C.c_double)), lat.data_ptr(), side,
                out.data_ptr(), ptr, nbytes, current_stream()))
            return out.cpu().numpy()  # (waits)

    def warp(self, src, A, phi, out_shape, interp="linear", default=0.0):
        """A tensor on the device (float32, or int32 for an integer source); no wait."""
        import torch

        if interp not in _abi.INTERPS:
            raise ValueError(f"interp must be 'linear' or 'nearest', got {interp!r}")
        t = src if is_tensor(src) else torch.from_numpy(np.ascontiguousarray(src))
        as_int = not (t.dtype.is_floating_point or t.dtype == torch.bool)
        if as_int and interp != "nearest":
            raise ValueError("an integer volume is warped with interp='nearest'")
        t = volume(t, torch.int32 if as_int else torch.float32, self.dev, "src")
        out_shape = tuple(int(v) for v in out_shape)
        a = _a12(A)
        with torch.cuda.device(self.dev):
            lat, side = self._lattice(phi)
            _, ptr, nbytes = self._workspace(out_shape, side)
            out = torch.empty(out_shape, dtype=t.dtype, device=self.dev)
            check(self.lib.t2fit_ffd_warp_dev(t.data_ptr(), _abi.RESAMPLE_I32 if as_int else _abi.RESAMPLE_F32, *t.shape,
                                              a.ctypes.data_as(C.POINTER(C.c_double)), lat.data_ptr(), side, out.data_ptr(), *out_shape,
                                              _abi.INTERPS[interp], float(default), ptr, nbytes, current_stream()))
            release(lat, t, self._workspace(out_shape, side)[0])
        return out

    def jacobian(self, phi, mask):
        import torch

        m = volume(mask, torch.uint8, self.dev, "mask")
        with torch.cuda.device(self.dev):
            lat, side = self._lattice(phi)
            _, ptr, nbytes = self._workspace(m.shape, side)
            out = torch.empty(2, dtype=torch.float64, device=self.dev)
            check(self.lib.t2fit_ffd_jacobian_dev(lat.data_ptr(), side, m.data_ptr(), *m.shape, out.data_ptr(), out.data_ptr() + 8, ptr,
                                                  nbytes, current_stream()))
            host = out.cpu().numpy()  # (waits)
        return float(host[0]), int(host.view(np.int64)[1])


def _pyramid(fixed_like, moving, fixed_mask, moving_mask, device, fixed_shape=None):
    import torch

    dev = pick_device((fixed_like, moving, fixed_mask, moving_mask), device)
    m = volume(moving, torch.float32, dev, "moving")
    shape = tuple(fixed_like.shape) if fixed_shape is None else fixed_shape
    f = torch.zeros(shape, dtype=torch.float32, device=dev)
    return DeviceFFDPyramid(f, _ones_like(f) if fixed_mask is None else fixed_mask, m, _ones_like(m) if moving_mask is None else moving_mask,
                            dev)


def ffd_joint_histogram(bins, moving, A, lattice, n_f, n_m, lo_m, scale_m, *, fixed_mask=None, moving_mask=None, device=0):
    """The joint histogram of Mattes mutual information under ``c(x) = A (x + d(x), 1)`` (t2fit_ffd_joint_hist_dev): uint64
    ``(n_f, n_m)``, numpy.  ``lattice``: float64 ``(3, c, c, c)``, ``c`` in (4, 5, 7, 11, 19), displacements in fixed voxels;
    None is zeros.  Integer for integer equal to :func:`_ffd.joint_histogram`, and with a lattice of zeros to
    ``register.joint_histogram``.  Waits for the stream."""
    dev = pick_device((bins, moving, fixed_mask, moving_mask), device)
    b = _bins_tensor(bins, dev)
    pyramid = _pyramid(b, moving, fixed_mask, moving_mask, device)
    return pyramid.hist(pyramid.full, b, n_f, n_m, lo_m, scale_m, A, _ffd.check_lattice(lattice))


def ffd_gradient(bins, table, moving, A, lattice, n_m, lo_m, scale_m, *, fixed_mask=None, moving_mask=None, side=None, device=0):
    """The lattice gradient of ``-MI`` with the counted set held fixed (t2fit_ffd_gradient_dev): float64 ``(3, c, c, c)``,
    numpy; ``table``: float64 ``(n_f, n_m)`` of :func:`_register.mattes_metric`.  ``lattice`` None: zeros of ``side``.
    Bit-identical to :func:`_ffd.gradient` and the same from call to call.  Waits for the stream."""
    dev = pick_device((bins, moving, fixed_mask, moving_mask), device)
    b = _bins_tensor(bins, dev)
    pyramid = _pyramid(b, moving, fixed_mask, moving_mask, device)
    return pyramid.gradient(pyramid.full, b, table, n_m, lo_m, scale_m, A, _ffd.check_lattice(lattice, side))


def ffd_warp(src, A, lattice, out_shape, *, interp="linear", default=0.0, device=0):
    """``src`` (float32, or an integer label volume that fits int32, with ``interp='nearest'``) sampled at ``c(x)`` on the
    fixed grid of ``out_shape`` (t2fit_ffd_warp_dev): numpy in, numpy out; a CUDA tensor in, a tensor out.  Bit-identical to
    :func:`_ffd.warp`; with a lattice of zeros (or None) the bytes of ``resample_volume`` for the same ``A``."""
    dev = pick_device((src,), device)
    pyramid = _pyramid(None, np.zeros((1, 1, 1), np.float32), None, None, dev.index, fixed_shape=(1, 1, 1))
    out = pyramid.warp(src, A, _ffd.check_lattice(lattice), out_shape, interp, default)
    return out if is_tensor(src) else out.cpu().numpy()


def ffd_min_jacobian(lattice, mask, *, device=0):
    """``(min det(I + dd/dx), count of det <= 0)`` over the voxels of ``mask`` (t2fit_ffd_jacobian_dev); ``(+inf, 0)`` for
    an empty mask.  Equal to :func:`_ffd.min_jacobian`.  Waits for the stream."""
    dev = pick_device((mask,), device)
    pyramid = _pyramid(None, np.zeros((1, 1, 1), np.float32), None, None, dev.index, fixed_shape=(1, 1, 1))
    return pyramid.jacobian(_ffd.check_lattice(lattice), mask)


def register_ffd(fixed, moving, fixed_geom, moving_geom, *, affine, fixed_mask=None, moving_mask=None, schedule=_ffd.DEFAULT_SCHEDULE,
                 bins=32, moving_bins=32, weight=_ffd.DEFAULT_WEIGHT, max_iter=_ffd.DEFAULT_MAX_ITER, max_step=_ffd.DEFAULT_MAX_STEP,
                 device=0):
    """Deform ``moving`` onto ``fixed`` (float32 ``(Z, Y, X)``, numpy or CUDA tensors) starting from ``affine``, the
    :class:`_register.Registration` of ``register_affine`` (or anything with a 4 x 4 ``transform``): a cubic B-spline
    free-form deformation ``c(x) = A (x + d(x), 1)`` on top of the affine, driven by Mattes mutual information (``bins``
    fixed, ``moving_bins`` moving bins) whatever metric found the affine, plus ``weight`` times the mean squared second
    difference of the lattice.  ``schedule``: ((shrink factor, lattice side), ..), sides from (4, 5, 7, 11, 19); between
    entries the lattice is subdivided and rescaled.  Regular-step descent per level from ``max_step`` voxels of the level,
    at most ``max_iter`` moves; the step is divided by the largest node-gradient norm, so no node moves further than the
    step.  The defaults of ``weight``, ``max_iter`` and ``max_step`` rest on one sweep on a phantom, nothing
    more.  Masks None: :func:`build_mask` on the device.  Returns an :class:`_ffd.FFDRegistration`: the affine (its
    ``transform`` / ``parameters``), ``lattice`` float64 ``(3, c, c, c)`` in full-resolution fixed voxels, per-level
    ``iterations`` and ``stops``, ``cost``, ``min_jacobian`` and ``n_folded`` (a folded result is reported, not refused).
    The histogram and the gradient of every iteration come from the GPU (two round trips per iteration); lattice,
    iterations, stops and cost equal :func:`_ffd.register_ffd`'s.  ValueError when a mask is empty or nothing overlaps.
    Parity with elastix, NiftyReg or ANTs is not pinned."""
    import torch

    dev = pick_device((fixed, moving, fixed_mask, moving_mask), device)
    f, m = volume(fixed, torch.float32, dev, "fixed"), volume(moving, torch.float32, dev, "moving")
    pyramid = DeviceFFDPyramid(f, build_mask(f, device=dev.index) if fixed_mask is None else fixed_mask,
                               m, build_mask(m, device=dev.index) if moving_mask is None else moving_mask, dev)
    fg, mg = _resample.as_geometry(fixed_geom, tuple(f.shape)), _resample.as_geometry(moving_geom, tuple(m.shape))
    schedule = _ffd.check_schedule(schedule, tuple(f.shape), tuple(m.shape))
    return _ffd.optimize_ffd(pyramid, fg, mg, affine, schedule=schedule, bins=bins, moving_bins=moving_bins, weight=weight,
                             max_iter=max_iter, max_step=max_step)
