"""Rigid and affine registration with the metric's sums on the GPU; :mod:`fetal_t2mapping_amd._register` states the sums
and the pyramid in numpy and holds the metric arithmetic and the optimizers, which run here unchanged."""
import ctypes as C

import numpy as np

from . import _abi, _register, _resample, _svr
from ._gpu import current_stream, pick_device, require, volume, workspace
from ._gpu_morph import build_mask
from ._lib import check


def _sums_workspace(lib, shape, dev):
    need = C.c_size_t(0)
    check(lib.t2fit_register_workspace_bytes(shape[0], shape[1], shape[2], C.byref(need)))
    ws, ptr = workspace(need.value, dev)
    return ws, ptr, need.value


class DevicePyramid:
    """The volumes and masks of every level as CUDA tensors, and their sums through t2fit_register_sums_dev: the two
    methods of :class:`_register.HostPyramid`.  ``sums`` copies 43 doubles to the host and so waits for the stream:
    once per iteration of the optimizer, which needs them to choose the next transform."""

    def __init__(self, fixed, fixed_mask, moving, moving_mask, dev):
        import torch

        self.lib = require(*_abi.REGISTER_SYMBOLS)
        self.dev = dev
        self.full = (volume(fixed, torch.float32, dev, "fixed"), volume(fixed_mask, torch.uint8, dev, "fixed_mask"),
                     volume(moving, torch.float32, dev, "moving"), volume(moving_mask, torch.uint8, dev, "moving_mask"))
        if self.full[0].shape != self.full[1].shape or self.full[2].shape != self.full[3].shape:
            raise ValueError("a mask has the shape of its volume")
        self.out = torch.empty(_abi.REGISTER_SUMS, dtype=torch.float64, device=dev)

    def _shrink(self, t, s):
        import torch

        out = torch.empty(_register.level_shape(t.shape, s), dtype=t.dtype, device=self.dev)
        fn = self.lib.t2fit_shrink_mask_dev if t.dtype == torch.uint8 else self.lib.t2fit_shrink_dev
        check(fn(t.data_ptr(), t.shape[0], t.shape[1], t.shape[2], int(s), out.data_ptr(), current_stream()))
        return out

    def level(self, s):
        import torch

        with torch.cuda.device(self.dev):
            tensors = self.full if s == 1 else tuple(self._shrink(t, s) for t in self.full)
            return tensors + _sums_workspace(self.lib, tensors[0].shape, self.dev)

    def sums(self, level, A):
        import torch

        fixed, fmask, moving, mmask, _, ptr, nbytes = level
        a = np.ascontiguousarray(A, np.float64).reshape(12)
        with torch.cuda.device(self.dev):
            check(self.lib.t2fit_register_sums_dev(fixed.data_ptr(), fmask.data_ptr(), *fixed.shape, moving.data_ptr(),
                                                   mmask.data_ptr(), *moving.shape, a.ctypes.data_as(C.POINTER(C.c_double)),
                                                   self.out.data_ptr(), ptr, nbytes, current_stream()))
            return self.out.cpu().numpy()  # (waits: the workspace and the tensors of the level are no longer in use)


def _bin_dev(lib, vol, lo, scale, n_bins, dev):
    import torch

    out = torch.empty(tuple(vol.shape), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.t2fit_register_bin_dev(vol.data_ptr(), vol.numel(), float(lo), float(scale), int(n_bins), out.data_ptr(),
                                         current_stream()))
    return out


def _bins_tensor(bins, dev):
    """A uint8 bin volume (values kept, unlike a mask) on ``dev``."""
    import torch

    if not (torch.is_tensor(bins) and bins.dtype == torch.uint8) and not (isinstance(bins, np.ndarray) and bins.dtype == np.uint8):
        raise ValueError("bins is a uint8 (Z, Y, X) volume")
    return volume(bins, torch.uint8, dev, "bins")


class DeviceAffinePyramid(DevicePyramid):
    """:class:`DevicePyramid` and the correlation ratio's steps, the methods of :class:`_register.HostAffinePyramid`.
    ``bins`` keeps a level's uint8 bin volume on the device (t2fit_register_bin_dev, once per level; the level's range
    inside its mask is read on the host, one copy of the level per level).  ``cr_sums`` queues
    t2fit_register_binned_sums_dev (N_b, S_b and the table) and t2fit_register_sums_lut_dev on the current stream -- no
    host step in between -- and copies ``2 n_bins + 43`` doubles back, which waits for the stream.  Mattes mutual
    information takes a round trip per evaluation: ``joint_hist`` (t2fit_register_joint_hist_dev) copies the ``n_f n_m``
    integers back, the host makes the metric and the table (:func:`_register.mattes_metric`), ``mi_sums`` uploads the
    table and copies the 12 sums of t2fit_register_mi_gradient_dev back."""

    def __init__(self, fixed, fixed_mask, moving, moving_mask, dev):
        super().__init__(fixed, fixed_mask, moving, moving_mask, dev)
        self.lib = require(*(_abi.REGISTER_SYMBOLS + _abi.ATLAS_SYMBOLS))
        self._bufs = {}
        self._mi_bufs = {}

    def bins(self, level, n_bins):
        lo, scale = _register.bin_range(level[0].cpu().numpy(), level[1].cpu().numpy(), n_bins)
        return _bin_dev(self.lib, level[0], lo, scale, n_bins, self.dev)

    def _buffers(self, shape, n_bins):
        """(results [2 B + B + 43] float64, binned workspace tensor, pointer, bytes) of a fixed shape and bin count."""
        import torch

        key = (tuple(shape), int(n_bins))
        if key not in self._bufs:
            need = C.c_size_t(0)
            check(self.lib.t2fit_register_binned_workspace_bytes(shape[0], shape[1], shape[2], int(n_bins), C.byref(need)))
            self._bufs = {key: (torch.empty(3 * n_bins + _abi.REGISTER_SUMS, dtype=torch.float64, device=self.dev),)
                          + workspace(need.value, self.dev) + (need.value,)}
        return self._bufs[key]

    def cr_sums(self, level, bins, n_bins, A):
        import torch

        _, fmask, moving, mmask, _, ptr, nbytes = level
        n_bins = int(n_bins)
        a = np.ascontiguousarray(A, np.float64).reshape(12)
        a_ptr = a.ctypes.data_as(C.POINTER(C.c_double))
        with torch.cuda.device(self.dev):
            out, _, bptr, bbytes = self._buffers(fmask.shape, n_bins)
            binned, lut, sums = out.data_ptr(), out.data_ptr() + 16 * n_bins, out.data_ptr() + 24 * n_bins
            st = current_stream()
            check(self.lib.t2fit_register_binned_sums_dev(bins.data_ptr(), fmask.data_ptr(), *fmask.shape, moving.data_ptr(),
                                                          mmask.data_ptr(), *moving.shape, a_ptr, n_bins, binned, lut, bptr, bbytes, st))
            check(self.lib.t2fit_register_sums_lut_dev(bins.data_ptr(), lut, n_bins, fmask.data_ptr(), *fmask.shape, moving.data_ptr(),
                                                       mmask.data_ptr(), *moving.shape, a_ptr, sums, ptr, nbytes, st))
            host = out.cpu().numpy()  # (waits)
        self.lut = host[2 * n_bins:3 * n_bins]
        return host[:2 * n_bins], host[3 * n_bins:]

    def moving_range(self, level, n_m):
        return _register.moving_bin_range(level[2].cpu().numpy(), level[3].cpu().numpy(), n_m)

    def _mi_buffers(self, shape, n_f, n_m):
        """(hist [n_f n_m] int64, table [n_f n_m] float64, sums [12] float64, workspace tensor, pointer, bytes)."""
        import torch

        key = (tuple(shape), int(n_f), int(n_m))
        if key not in self._mi_bufs:
            lib = require(*_abi.MI_SYMBOLS)
            need = C.c_size_t(0)
            check(lib.t2fit_register_mi_workspace_bytes(shape[0], shape[1], shape[2], C.byref(need)))
            self._mi_bufs = {key: (torch.empty(n_f * n_m, dtype=torch.int64, device=self.dev),
                                   torch.empty(n_f * n_m, dtype=torch.float64, device=self.dev),
                                   torch.empty(_abi.REGISTER_MI_SUMS, dtype=torch.float64, device=self.dev))
                             + workspace(need.value, self.dev) + (need.value,)}
        return self._mi_bufs[key]

    def joint_hist(self, level, bins, n_f, n_m, lo_m, scale_m, A):
        import torch

        _, fmask, moving, mmask = level[:4]
        n_f, n_m = _register._check_bins(n_f), _register._check_moving_bins(n_m)
        a = np.ascontiguousarray(A, np.float64).reshape(12)
        with torch.cuda.device(self.dev):
            hist = self._mi_buffers(fmask.shape, n_f, n_m)[0]
            check(require(*_abi.MI_SYMBOLS).t2fit_register_joint_hist_dev(
                bins.data_ptr(), fmask.data_ptr(), *fmask.shape, moving.data_ptr(), mmask.data_ptr(), *moving.shape,
                a.ctypes.data_as(C.POINTER(C.c_double)), n_f, n_m, float(lo_m), float(scale_m), hist.data_ptr(), current_stream()))
            return hist.cpu().numpy().view(np.uint64).reshape(n_f, n_m)  # (waits)

    def mi_sums(self, level, bins, table, n_m, lo_m, scale_m, A):
        import torch

        _, fmask, moving, mmask = level[:4]
        table = np.ascontiguousarray(table, np.float64)
        if table.ndim != 2 or table.shape[1] != int(n_m):
            raise ValueError("table is float64 (n_f, n_m)")
        n_f, n_m = _register._check_bins(table.shape[0]), _register._check_moving_bins(n_m)
        a = np.ascontiguousarray(A, np.float64).reshape(12)
        with torch.cuda.device(self.dev):
            _, table_dev, sums, _, ptr, nbytes = self._mi_buffers(fmask.shape, n_f, n_m)
            table_dev.copy_(torch.from_numpy(table.ravel()))  # (pageable memory: the copy has left the host when it returns)
            check(require(*_abi.MI_SYMBOLS).t2fit_register_mi_gradient_dev(
                bins.data_ptr(), table_dev.data_ptr(), n_f, n_m, float(lo_m), float(scale_m), fmask.data_ptr(), *fmask.shape,
                moving.data_ptr(), mmask.data_ptr(), *moving.shape, a.ctypes.data_as(C.POINTER(C.c_double)), sums.data_ptr(), ptr,
                nbytes, current_stream()))
            return sums.cpu().numpy()  # (waits)


def _ones_like(t):
    import torch

    return torch.ones(tuple(t.shape), dtype=torch.uint8, device=t.device)


def registration_sums(fixed, moving, A, *, fixed_mask=None, moving_mask=None, device=0):
    """The 43 float64 sums of the correlation metric and its gradient with respect to the index affine ``A`` (fixed index
    -> continuous moving index, :func:`_resample.index_affine`), as a numpy array: ``[N, sum f, sum m, sum ff, sum mm,
    sum fm, 36 gradient sums]`` in the order of include/t2fit.h.  ``fixed`` / ``moving``: float32 ``(Z, Y, X)`` numpy
    arrays or CUDA tensors; masks 0 / not 0, None: all ones.  Bit-identical to :func:`_register.registration_sums` and
    the same from call to call.  ``N = 0`` returns 43 zeros.  Waits for the stream (the copy of the result)."""
    import torch

    dev = pick_device((fixed, moving, fixed_mask, moving_mask), device)
    f, m = volume(fixed, torch.float32, dev, "fixed"), volume(moving, torch.float32, dev, "moving")
    pyramid = DevicePyramid(f, _ones_like(f) if fixed_mask is None else fixed_mask, m,
                            _ones_like(m) if moving_mask is None else moving_mask, dev)
    return pyramid.sums(pyramid.level(1), A)


def register_rigid(fixed, moving, fixed_geom, moving_geom, *, fixed_mask=None, moving_mask=None, levels=(4, 2, 1), max_iter=100,
                   init=None, metric="corr", bins=32, moving_bins=32, device=0):  # noqa: A002
    """Register ``moving`` onto ``fixed``: float32 ``(Z, Y, X)`` volumes (numpy or CUDA tensors) with their geometries
    (anything with GetSpacing / GetOrigin / GetDirection).  The recipe is the reference's ``registration_itk``
    (utils/qmri_utils.py:167-221) made deterministic: correlation metric over every voxel of the fixed mask whose image
    falls into the moving mask, linear interpolation, Euler angles about the fixed mask's centroid, regular-step
    gradient descent (first step 1 mm times the level's shrink factor, halved when the gradient turns, stops at step
    1e-6, gradient 1e-6 or ``max_iter`` iterations per level), rotation scales from the mask's mean squared radius, a
    pyramid of block means (``levels``: integer shrink factors).  Masks None: :func:`build_mask` of the volume, on the
    device.  ``init``: (rx, ry, rz [rad], tx, ty, tz [mm]).  Returns a :class:`_register.Registration`: ``.transform`` is
    the 4 x 4 (fixed point -> moving point, LPS mm) that ``reconstruct_stacks(transforms=)``, ``resample_volume(
    transform=)`` and ``recon.py --transforms`` take.  The sums of every iteration come from the GPU and one 43-double
    copy per iteration waits for the stream; parameters, iteration counts and stop reasons equal
    :func:`_register.register_rigid`'s.  ``metric='mattes'``: Mattes mutual information in place of the correlation, by
    :func:`register_affine` with 6 degrees of freedom (``bins``, ``moving_bins``); the result keeps this function's
    shape, six parameters.  ValueError when the masks do not overlap.  Parity with elastix is not pinned."""
    import torch

    if _register.check_rigid_metric(metric) == "mattes":
        return _register.rigid_from_affine(register_affine(
            fixed, moving, fixed_geom, moving_geom, metric="mattes", bins=bins, moving_bins=moving_bins, dof=6, fixed_mask=fixed_mask,
            moving_mask=moving_mask, levels=levels, max_iter=max_iter, init=_register.rigid_init(init), device=device))
    dev = pick_device((fixed, moving, fixed_mask, moving_mask), device)
    f, m = volume(fixed, torch.float32, dev, "fixed"), volume(moving, torch.float32, dev, "moving")
    pyramid = DevicePyramid(f, build_mask(f, device=dev.index) if fixed_mask is None else fixed_mask,
                            m, build_mask(m, device=dev.index) if moving_mask is None else moving_mask, dev)
    fg, mg = _resample.as_geometry(fixed_geom, tuple(f.shape)), _resample.as_geometry(moving_geom, tuple(m.shape))
    levels = _register.check_levels(levels, tuple(f.shape), tuple(m.shape))
    centre, scales = _register.mask_centre_and_scales(pyramid.full[1].cpu().numpy(), fg)  # one mask to the host, once
    return _register.optimize(pyramid, fg, mg, centre, scales, levels=levels, max_iter=max_iter, init=init)


def _affine_pyramid(fixed, moving, fixed_mask, moving_mask, device):
    import torch

    dev = pick_device((fixed, moving, fixed_mask, moving_mask), device)
    f, m = volume(fixed, torch.float32, dev, "fixed"), volume(moving, torch.float32, dev, "moving")
    return DeviceAffinePyramid(f, _ones_like(f) if fixed_mask is None else fixed_mask, m,
                               _ones_like(m) if moving_mask is None else moving_mask, dev)


def bin_volume(vol, lo, scale, n_bins, *, device=0):
    """uint8 CUDA tensor ``clamp(floor((float64(vol) - lo) * scale), 0, n_bins - 1)``, NaN -> 0 (t2fit_register_bin_dev):
    bit-identical to :func:`_register.bin_volume`."""
    import torch

    dev = pick_device((vol,), device)
    return _bin_dev(require(*_abi.ATLAS_SYMBOLS), volume(vol, torch.float32, dev, "vol"), lo, scale, n_bins, dev)


def binned_sums(bins, moving, A, n_bins, *, fixed_mask=None, moving_mask=None, device=0, return_lut=False):
    """``N_b`` then ``S_b`` (float64 ``[2 n_bins]``, numpy) of ``moving`` sampled at ``A`` over the uint8 ``bins`` volume
    of the fixed grid; with ``return_lut`` also ``lut[b] = S_b / N_b``.  Bit-identical to :func:`_register.binned_sums`
    and :func:`_register.lut_from_binned`, and the same from call to call.  Waits for the stream."""
    import torch

    dev = pick_device((bins, moving, fixed_mask, moving_mask), device)
    b = _bins_tensor(bins, dev)
    pyramid = _affine_pyramid(torch.zeros(tuple(b.shape), dtype=torch.float32, device=dev), moving, fixed_mask, moving_mask, device)
    binned, _ = pyramid.cr_sums(pyramid.level(1), b, n_bins, A)
    return (binned, pyramid.lut) if return_lut else binned


def registration_sums_lut(bins, lut, moving, A, *, fixed_mask=None, moving_mask=None, device=0):
    """The 43 sums with ``f = lut[bins]`` (float64, not rounded to float32; t2fit_register_sums_lut_dev): bit-identical
    to :func:`_register.registration_sums_lut`.  Waits for the stream."""
    import torch

    dev = pick_device((bins, moving, fixed_mask, moving_mask), device)
    b = _bins_tensor(bins, dev)
    table = torch.from_numpy(np.ascontiguousarray(lut, np.float64).ravel()).to(dev)
    pyramid = _affine_pyramid(torch.zeros(tuple(b.shape), dtype=torch.float32, device=dev), moving, fixed_mask, moving_mask, device)
    _, fmask, m, mmask, _, ptr, nbytes = pyramid.level(1)
    a = np.ascontiguousarray(A, np.float64).reshape(12)
    with torch.cuda.device(dev):
        check(pyramid.lib.t2fit_register_sums_lut_dev(b.data_ptr(), table.data_ptr(), table.numel(), fmask.data_ptr(), *fmask.shape,
                                                      m.data_ptr(), mmask.data_ptr(), *m.shape, a.ctypes.data_as(C.POINTER(C.c_double)),
                                                      pyramid.out.data_ptr(), ptr, nbytes, current_stream()))
        return pyramid.out.cpu().numpy()


def joint_histogram(bins, moving, A, n_f, n_m, lo_m, scale_m, *, fixed_mask=None, moving_mask=None, device=0):
    """The joint histogram of Mattes mutual information (t2fit_register_joint_hist_dev): uint64 ``(n_f, n_m)``, numpy.  A
    counted voxel of fixed bin ``b`` (the uint8 ``bins`` volume, ``n_f`` in 1..64) adds the four cubic B-spline window
    weights of its interpolated moving sample, in units of 2^-30, to row ``b`` (``n_m`` in 5..64 moving bins over
    ``lo_m`` .. with ``scale_m``: :func:`_register.moving_bin_range`).  Integer for integer equal to
    :func:`_register.joint_histogram` and the same from call to call.  Waits for the stream."""
    import torch

    dev = pick_device((bins, moving, fixed_mask, moving_mask), device)
    b = _bins_tensor(bins, dev)
    pyramid = _affine_pyramid(torch.zeros(tuple(b.shape), dtype=torch.float32, device=dev), moving, fixed_mask, moving_mask, device)
    return pyramid.joint_hist(pyramid.level(1), b, n_f, n_m, lo_m, scale_m, A)


def mi_gradient_sums(bins, table, moving, A, n_m, lo_m, scale_m, *, fixed_mask=None, moving_mask=None, device=0):
    """The 12 float64 sums ``[4 a + j] = sum (c g_a) u_j`` of t2fit_register_mi_gradient_dev, numpy; ``table``: float64
    ``(n_f, n_m)``, with :func:`_register.mattes_metric`'s they are ``d(-MI)/dA``.  Bit-identical to
    :func:`_register.mi_gradient_sums`.  Waits for the stream."""
    import torch

    dev = pick_device((bins, moving, fixed_mask, moving_mask), device)
    b = _bins_tensor(bins, dev)
    pyramid = _affine_pyramid(torch.zeros(tuple(b.shape), dtype=torch.float32, device=dev), moving, fixed_mask, moving_mask, device)
    return pyramid.mi_sums(pyramid.level(1), b, table, n_m, lo_m, scale_m, A)


def register_affine(fixed, moving, fixed_geom, moving_geom, *, metric="cr", bins=32, dof=12, fixed_mask=None, moving_mask=None,  # noqa: A002
                    levels=(4, 2, 1), max_iter=100, init=None, moving_bins=32, device=0):
    """Register ``moving`` onto ``fixed`` with ``dof`` in (6, 7, 9, 12) degrees of freedom: ``x' = R K (x - centre) +
    centre + t`` (:func:`_register.compose_affine`: Euler angles, translation, log scales, shears) by the regular-step
    descent of :func:`register_rigid`.  ``metric='cr'``: the correlation ratio of the moving samples given the fixed
    volume binned into ``bins`` (1..64) bins -- what the reference asks of FSL's flirt for the T1 template onto a T2w
    volume; each level's bins span that level's fixed samples inside its mask.  ``'ncc'``: the squared correlation of
    :func:`register_rigid`.  ``'mattes'``: Mattes mutual information, the cost elastix's default rigid map minimises --
    ``bins`` fixed bins (a zero-order window) and ``moving_bins`` (5..64) cubic B-spline bins over each level's moving
    samples inside its mask, every counted voxel sampled; parity with elastix (random samples, another descent) is not
    pinned.  ``init``: None, 12 parameters, or 'centroids' (start at the translation between the masks'
    centroids: a template and a subject do not share a frame).  Masks None: :func:`build_mask` on the device.  Returns a
    :class:`_register.Registration` with 12 parameters; they, the iteration counts and the stops equal
    :func:`_register.register_affine`'s.  Parity with flirt (another optimizer, another search) is not pinned."""
    import torch

    dev = pick_device((fixed, moving, fixed_mask, moving_mask), device)
    f, m = volume(fixed, torch.float32, dev, "fixed"), volume(moving, torch.float32, dev, "moving")
    pyramid = DeviceAffinePyramid(f, build_mask(f, device=dev.index) if fixed_mask is None else fixed_mask,
                                  m, build_mask(m, device=dev.index) if moving_mask is None else moving_mask, dev)
    fg, mg = _resample.as_geometry(fixed_geom, tuple(f.shape)), _resample.as_geometry(moving_geom, tuple(m.shape))
    levels = _register.check_levels(levels, tuple(f.shape), tuple(m.shape))
    fmask_host = pyramid.full[1].cpu().numpy()
    centre, scales = _register.affine_centre_and_scales(fmask_host, fg)
    p0 = _register.affine_init(init, fmask_host, fg, pyramid.full[3].cpu().numpy() if isinstance(init, str) else None, mg)
    return _register.optimize_affine(pyramid, fg, mg, centre, scales, metric=metric, bins=bins, dof=dof, levels=levels,
                                     max_iter=max_iter, init=p0, moving_bins=moving_bins)


# ---- slice-to-volume registration ------------------------------------------------------------------------------------------
_as_volume = volume  # (the functions below have an argument of that name)


class DeviceSlices:
    """The stacks, their masks, the volume and its mask as CUDA tensors, with the table, the sums and the workspace of
    t2fit_svr_sums_dev sized for ``n_slices`` records: everything stays on the device; ``sums`` uploads the packed table
    (128 bytes a record) and downloads ``(K, 43)`` doubles, which waits for the stream."""

    def __init__(self, stacks, stack_masks, moving, moving_mask, n_slices, dev):
        import torch

        self.lib = require(*_abi.SVR_SYMBOLS)
        self.dev = dev
        if not 1 <= len(stacks) <= _abi.SR_MAX_STACKS:
            raise ValueError(f"between 1 and {_abi.SR_MAX_STACKS} stacks, got {len(stacks)}")
        stack_masks = [None] * len(stacks) if stack_masks is None else list(stack_masks)
        if len(stack_masks) != len(stacks):
            raise ValueError("one mask (or None) per stack")
        self.stacks = [volume(v, torch.float32, dev, "a stack") for v in stacks]
        self.masks = [None if m is None else volume(m, torch.uint8, dev, "a stack mask") for m in stack_masks]
        self.moving = volume(moving, torch.float32, dev, "volume")
        self.moving_mask = None if moving_mask is None else volume(moving_mask, torch.uint8, dev, "volume_mask")
        if any(m is not None and m.shape != v.shape for v, m in zip(self.stacks, self.masks)) or (
                self.moving_mask is not None and self.moving_mask.shape != self.moving.shape):
            raise ValueError("a mask has the shape of its volume")
        self.n = int(n_slices)
        n_s = len(self.stacks)
        self.shapes = [tuple(int(d) for d in v.shape) for v in self.stacks]
        self.lo_size = (C.c_int32 * (3 * n_s))(*[d for s in self.shapes for d in s])
        self.fixed_ptrs = (C.c_void_p * n_s)(*[v.data_ptr() for v in self.stacks])
        self.mask_ptrs = (C.c_void_p * n_s)(*[None if m is None else m.data_ptr() for m in self.masks])
        need, table = C.c_size_t(0), C.c_size_t(0)
        check(self.lib.t2fit_svr_workspace_bytes(n_s, self.lo_size, self.n, C.byref(need)))
        check(self.lib.t2fit_svr_table_bytes(self.n, C.byref(table)))
        with torch.cuda.device(dev):
            self.ws, self.ws_ptr = workspace(need.value, dev)
            self.ws_bytes = need.value
            self.table = torch.empty(table.value, dtype=torch.uint8, device=dev)
            self.out = torch.empty((self.n, _abi.REGISTER_SUMS), dtype=torch.float64, device=dev)
        self.table_host = np.zeros(table.value, np.uint8)

    def sums(self, A, stack, slice_, active=None):
        a, s, k, act = _svr.check_records(A, stack, slice_, active)
        if len(a) != self.n:
            raise ValueError(f"{self.n} records were planned, got {len(a)}")
        # (the packing refuses a non-finite A and an index out of range before a byte is written)
        check(self.lib.t2fit_svr_table_host(self.n, a.ctypes.data_as(C.POINTER(C.c_double)), s.ctypes.data_as(C.POINTER(C.c_int32)),
                                            k.ctypes.data_as(C.POINTER(C.c_int32)), act.ctypes.data_as(C.POINTER(C.c_uint8)),
                                            len(self.stacks), self.lo_size, self.table_host.ctypes.data_as(C.c_void_p),
                                            self.table_host.size))
        return self.sums_of_table(self.table_host)

    def sums_of_table(self, table_bytes):
        """The sums of a packed table (uint8 ``[128 K]``, taken as data: whatever it holds)."""
        import torch

        with torch.cuda.device(self.dev):
            self.table.copy_(torch.from_numpy(np.ascontiguousarray(table_bytes, np.uint8).reshape(-1)))  # (pageable: the copy has left the host)
            check(self.lib.t2fit_svr_sums_dev(len(self.stacks), self.fixed_ptrs, self.mask_ptrs, self.lo_size, self.moving.data_ptr(),
                                              None if self.moving_mask is None else self.moving_mask.data_ptr(), *self.moving.shape,
                                              self.table.data_ptr(), self.n, self.out.data_ptr(), self.ws_ptr, self.ws_bytes,
                                              current_stream()))
            return self.out.cpu().numpy()  # (waits)


def slice_sums(stacks, volume, A, stack, slice_, *, active=None, stack_masks=None, volume_mask=None, device=0):  # noqa: A002
    """float64 ``(K, 43)``, numpy: the 43 sums of the correlation metric of record ``r`` = slice ``slice_[r]`` of
    ``stacks[stack[r]]`` (a list of float32 ``(Z, Y, X)``, numpy or CUDA tensors) sampled from ``volume`` at its own index
    affine ``A[r]`` (slice index ``(ix, iy, k)`` -> continuous volume index), all in one launch (t2fit_svr_sums_dev).
    ``active``: 0 gives a row of zeros; masks None: all ones.  Refuses a non-finite ``A`` and an index out of range.
    Bit-identical to :func:`_svr.slice_sums` and the same from call to call.  Waits for the stream."""
    dev = pick_device(list(stacks) + [volume, volume_mask], device)
    n = len(np.asarray(stack).ravel())
    return DeviceSlices(stacks, stack_masks, volume, volume_mask, n, dev).sums(A, stack, slice_, active)


def register_slices(stacks, geoms, volume, volume_geom, *, transforms=None, stack_masks=None, volume_mask=None, echo=0, init=None,  # noqa: A002
                    max_iter=_svr.MAX_ITER, step=_svr.STEP, min_step=_svr.MIN_STEP, min_count=_svr.MIN_COUNT, device=0):
    """Slice-to-volume registration: every slice of every stack is registered rigidly onto ``volume`` with the correlation
    metric, and the poses ``reconstruct_sr(slice_transforms=)`` takes come back.  ``stacks`` / ``geoms``: {name: float32
    ``(Z, Y, X)`` or ``(nTE, Z, Y, X)`` (``echo`` is used), numpy or CUDA tensors} and their geometries; ``volume``:
    float32 ``(Z, Y, X)`` on ``volume_geom``; ``transforms``: {name: 4 x 4 stack transform, fixed point -> stack point};
    ``stack_masks``: {name: ``(Z, Y, X)``}, a stack without one gets :func:`build_mask` on the device; ``volume_mask``:
    None is all ones; ``init``: {name: ``(lz, 6)``} parameters to start from.  Slice ``k`` moves by ``p = (rx, ry, rz [rad],
    tx, ty, tz [mm])`` about the centroid of its own mask, regular-step descent from ``step`` mm (halved when the gradient
    turns; stops at ``min_step``, gradient 1e-6 or ``max_iter`` moves), one full-resolution level; all slices advance in
    lockstep with one batched evaluation per iteration (t2fit_svr_sums_dev: a 128-byte record per slice up, 43 doubles per
    slice down), a finished slice is no longer evaluated.  No slice makes the call raise: fewer than ``min_count``
    counted voxels or no metric at the first evaluation is status 'rejected' (the stack's own pose), later 'lost' (the last
    pose that had a metric).  Returns a :class:`_svr.SliceRegistration`; parameters, iterations and status equal
    :func:`_svr.register_slices`'s."""
    import torch

    _svr.check_options(max_iter, step, min_step, min_count)
    names = _svr._stack_names(stacks, geoms)
    dev = pick_device([stacks[o] for o in names] + [volume, volume_mask], device)
    ys = []
    for o in names:
        v = stacks[o] if torch.is_tensor(stacks[o]) else np.asarray(stacks[o], np.float32)
        if len(v.shape) not in (3, 4):
            raise ValueError(f"stack {o!r} must be (Z, Y, X) or (nTE, Z, Y, X), got shape {tuple(v.shape)}")
        ys.append(_as_volume(v if len(v.shape) == 3 else v[int(echo)], torch.float32, dev, f"stack {o!r}"))
    stack_masks = stack_masks or {}
    masks = [build_mask(y, device=dev.index) if stack_masks.get(o) is None else stack_masks[o] for o, y in zip(names, ys)]
    lzs = [int(y.shape[0]) for y in ys]
    slices = DeviceSlices(ys, masks, volume, volume_mask, sum(lzs), dev)
    s_of = np.array([s for s, lz in enumerate(lzs) for _ in range(lz)], np.int32)
    k_of = np.array([k for lz in lzs for k in range(lz)], np.int32)
    host_masks = [m.cpu().numpy() for m in slices.masks]  # the masks to the host, once: centres and scales
    return _svr.register_with(lambda a, active: slices.sums(a, s_of, k_of, active), names, geoms, host_masks,
                              _resample.as_geometry(volume_geom, tuple(slices.moving.shape)), transforms, init,
                              max_iter=int(max_iter), step=float(step), min_step=float(min_step), min_count=int(min_count))


# ---- non-rigid alignment ---------------------------------------------------------------------------------------------------
_FFD_NAMES = ("register_ffd", "ffd_joint_histogram", "ffd_gradient", "ffd_warp", "ffd_min_jacobian")


def __getattr__(name):
    """``register.register_ffd`` and the four ``ffd_*`` steps live in :mod:`_gpu_ffd`, which builds on this module."""
    if name in _FFD_NAMES:
        from . import _gpu_ffd

        return getattr(_gpu_ffd, name)
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
