"""Rigid registration with the metric's sums on the GPU; :mod:`fetal_t2mapping_amd._register` states the sums and the
pyramid in numpy and holds the metric arithmetic and the optimizer, which run here unchanged."""
import ctypes as C

import numpy as np

from . import _abi, _register, _resample
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
                   init=None, device=0):
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
    :func:`_register.register_rigid`'s.  ValueError when the masks do not overlap.  Parity with elastix is not pinned."""
    import torch

    dev = pick_device((fixed, moving, fixed_mask, moving_mask), device)
    f, m = volume(fixed, torch.float32, dev, "fixed"), volume(moving, torch.float32, dev, "moving")
    pyramid = DevicePyramid(f, build_mask(f, device=dev.index) if fixed_mask is None else fixed_mask,
                            m, build_mask(m, device=dev.index) if moving_mask is None else moving_mask, dev)
    fg, mg = _resample.as_geometry(fixed_geom, tuple(f.shape)), _resample.as_geometry(moving_geom, tuple(m.shape))
    levels = _register.check_levels(levels, tuple(f.shape), tuple(m.shape))
    centre, scales = _register.mask_centre_and_scales(pyramid.full[1].cpu().numpy(), fg)  # one mask to the host, once
    return _register.optimize(pyramid, fg, mg, centre, scales, levels=levels, max_iter=max_iter, init=init)
