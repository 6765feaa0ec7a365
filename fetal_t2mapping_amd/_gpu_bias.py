"""N4 bias-field correction with every per-voxel step on the GPU; :mod:`fetal_t2mapping_amd._bias` states the steps in
numpy and holds the sharpening table, the lattice refinement and the loop, which run here unchanged."""
import ctypes as C

import numpy as np

from . import _abi, _bias
from ._bias import N4Result  # noqa: F401
from ._gpu import current_stream, is_tensor, pick_device, require, volume, workspace
from ._gpu_morph import build_mask
from ._lib import check


def _lib():
    return require(*_abi.N4_SYMBOLS)


def _workspace(lib, shape, side, dev):
    need = C.c_size_t(0)
    check(lib.t2fit_n4_workspace_bytes(int(shape[0]), int(shape[1]), int(shape[2]), int(side), C.byref(need)))
    ws, ptr = workspace(need.value, dev)
    return ws, ptr, need.value


def _side(lattice):
    lattice = np.asarray(lattice, np.float64)
    if lattice.ndim != 3 or len(set(lattice.shape)) != 1 or lattice.shape[0] not in _bias.SIDES:
        raise ValueError(f"the lattice is a cube of side {_bias.SIDES}, got shape {lattice.shape}")
    return lattice.shape[0]


def _out(t, like):
    """A result as the caller handed the volume in: a tensor for a tensor, else numpy."""
    return t if is_tensor(like) else t.cpu().numpy()


# ---- the steps, one entry point each (the tests call these) --------------------------------------------------------------
def log_image(vol, mask=None, *, device=0):
    """``(u0, M)``: float32 ``log`` of ``vol`` where ``mask`` (None: everywhere) and ``vol > 0``, +0.0 elsewhere, and that
    mask as uint8 (t2fit_n4_log_dev).  CUDA tensors.  M equals :func:`_bias.log_image`'s; ``u0`` is within 1 float32 ulp."""
    import torch

    lib = _lib()
    dev = pick_device((vol, mask), device)
    v = volume(vol, torch.float32, dev)
    m_in = None if mask is None else volume(mask, torch.uint8, dev, "mask")
    if m_in is not None and m_in.shape != v.shape:
        raise ValueError("the mask has the shape of the volume")
    u0, m = torch.empty_like(v), torch.empty(tuple(v.shape), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        check(lib.t2fit_n4_log_dev(v.data_ptr(), None if m_in is None else m_in.data_ptr(), v.numel(), u0.data_ptr(), m.data_ptr(),
                                   current_stream()))
    return u0, m


def minmax(u, m, *, device=0):
    """(lo, hi) float32 of ``u`` over ``m`` (t2fit_n4_minmax_dev): equal to :func:`_bias.minmax`.  Waits for the stream."""
    import torch

    lib = _lib()
    dev = pick_device((u, m), device)
    ut, mt = volume(u, torch.float32, dev, "u"), volume(m, torch.uint8, dev, "m")
    out = torch.empty(2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws, ptr = workspace(8192, dev)
        check(lib.t2fit_n4_minmax_dev(ut.data_ptr(), mt.data_ptr(), ut.numel(), out.data_ptr(), ptr, 8192, current_stream()))
        lo, hi = out.cpu().numpy()
    return lo, hi


def histogram(u, m, lo, slope, bins=_bias.BINS, *, device=0):
    """uint64 ``[bins]`` numpy (t2fit_n4_histogram_dev): equal to :func:`_bias.histogram`.  Waits for the stream."""
    import torch

    lib = _lib()
    dev = pick_device((u, m), device)
    ut, mt = volume(u, torch.float32, dev, "u"), volume(m, torch.uint8, dev, "m")
    out = torch.empty(int(bins), dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        check(lib.t2fit_n4_histogram_dev(ut.data_ptr(), mt.data_ptr(), ut.numel(), float(lo), float(slope), int(bins), out.data_ptr(),
                                         current_stream()))
        return out.cpu().numpy().view(np.uint64)


def fit_weights(m, side, *, device=0):
    """``omega`` float64 ``[c, c, c]`` numpy (t2fit_n4_weights_dev): bit-identical to :func:`_bias.fit_weights`."""
    import torch

    lib = _lib()
    dev = pick_device((m,), device)
    mt = volume(m, torch.uint8, dev, "m")
    out = torch.empty((side,) * 3, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        ws, ptr, nbytes = _workspace(lib, mt.shape, side, dev)
        check(lib.t2fit_n4_weights_dev(mt.data_ptr(), *mt.shape, int(side), out.data_ptr(), ptr, nbytes, current_stream()))
        return out.cpu().numpy()


def fit(u, m, lattice, omega, table=None, lo=0.0, slope=1.0, *, device=0):
    """``(delta, lattice + delta / omega)`` float64 numpy (t2fit_n4_fit_dev); ``table`` None fits ``u`` itself.
    Bit-identical to :func:`_bias.fit_delta` and :func:`_bias.lattice_update`."""
    import torch

    lib = _lib()
    dev = pick_device((u, m), device)
    ut, mt = volume(u, torch.float32, dev, "u"), volume(m, torch.uint8, dev, "m")
    side = _side(lattice)
    lat = torch.from_numpy(np.ascontiguousarray(lattice, np.float64)).to(dev)
    om = torch.from_numpy(np.ascontiguousarray(omega, np.float64).reshape((side,) * 3)).to(dev)
    tab = None if table is None else torch.from_numpy(np.ascontiguousarray(table, np.float64).ravel()).to(dev)
    delta = torch.empty_like(lat)
    with torch.cuda.device(dev):
        ws, ptr, nbytes = _workspace(lib, ut.shape, side, dev)
        check(lib.t2fit_n4_fit_dev(ut.data_ptr(), mt.data_ptr(), *ut.shape, None if tab is None else tab.data_ptr(), float(lo),
                                   float(slope), 2 if tab is None else tab.numel(), side, om.data_ptr(), lat.data_ptr(),
                                   delta.data_ptr(), ptr, nbytes, current_stream()))
        return delta.cpu().numpy(), lat.cpu().numpy()


def field_step(lattice, u0, m, field_old=None, *, device=0):
    """``(field, u, (sum d, sum d^2), (lo, hi))`` of a lattice (t2fit_n4_field_dev): the float32 field at every voxel and
    the new ``u = u0 - field`` as CUDA tensors, the convergence sums against ``field_old`` (None: zeros) and the range of
    the new ``u`` over ``m`` as numpy.  The field, ``u`` and the range equal :func:`_bias.field_eval`, :func:`_bias.next_u`
    and :func:`_bias.minmax` bit for bit; the sums pass through ``expm1``."""
    import torch

    lib = _lib()
    dev = pick_device((u0, m, field_old), device)
    u0t, mt = volume(u0, torch.float32, dev, "u0"), volume(m, torch.uint8, dev, "m")
    side = _side(lattice)
    lat = torch.from_numpy(np.ascontiguousarray(lattice, np.float64)).to(dev)
    field = torch.zeros_like(u0t) if field_old is None else volume(field_old, torch.float32, dev, "field_old").clone()
    u = torch.empty_like(u0t)
    sums, rng = torch.empty(2, dtype=torch.float64, device=dev), torch.empty(2, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        ws, ptr, nbytes = _workspace(lib, u0t.shape, side, dev)
        check(lib.t2fit_n4_field_dev(lat.data_ptr(), side, u0t.data_ptr(), mt.data_ptr(), *u0t.shape, field.data_ptr(), u.data_ptr(),
                                     sums.data_ptr(), rng.data_ptr(), ptr, nbytes, current_stream()))
        return field, u, tuple(sums.cpu().numpy()), tuple(rng.cpu().numpy())


def apply_field(volume_in, log_field, scale=1.0, *, device=0):
    """``float32(float64(volume) / exp(float64(log_field)) * scale)`` (t2fit_n4_apply_dev): divide any echo by a field
    estimated on another.  numpy in, numpy out; a CUDA tensor in, a tensor out.  Within 1 float32 ulp of
    :func:`_bias.apply_field`."""
    import torch

    lib = _lib()
    dev = pick_device((volume_in, log_field), device)
    v, f = volume(volume_in, torch.float32, dev), volume(log_field, torch.float32, dev, "log_field")
    if v.shape != f.shape:
        raise ValueError("the field has the shape of the volume")
    out = torch.empty_like(v)
    with torch.cuda.device(dev):
        check(lib.t2fit_n4_apply_dev(v.data_ptr(), f.data_ptr(), v.numel(), float(scale), out.data_ptr(), current_stream()))
    return _out(out, volume_in)


# ---- the whole call ------------------------------------------------------------------------------------------------------
class DeviceSteps:
    """The methods of :class:`_bias.HostSteps` with the kernels in place of the numpy steps.  The volumes, the lattice
    and omega stay on the device; per iteration the histogram (``bins`` uint64) and the sums (two doubles, two floats)
    come to the host and the table (``bins`` doubles) goes to the device: the table is host arithmetic on the histogram,
    and the loop needs the figure to decide whether to go on."""

    def __init__(self, vol, mask, dev):
        import torch

        self.lib, self.dev = _lib(), dev
        self.vol = volume(vol, torch.float32, dev)
        if not bool(torch.isfinite(self.vol).all()):
            raise ValueError("N4: the volume must be finite")
        self.u0, self.m = log_image(self.vol, mask)
        self.u = self.u0.clone()
        self.field = torch.zeros_like(self.u0)
        self.sums = torch.empty(2, dtype=torch.float64, device=dev)
        self.rng = torch.empty(2, dtype=torch.float32, device=dev)
        self.hist = torch.empty(_bias.MAX_BINS, dtype=torch.int64, device=dev)
        self.table = torch.empty(_bias.MAX_BINS, dtype=torch.float64, device=dev)
        self.side = None

    def range(self):  # noqa: A003
        return minmax(self.u, self.m)

    def set_level(self, lattice):
        import torch

        self.side = _side(lattice)
        self.lat = torch.from_numpy(np.ascontiguousarray(lattice, np.float64)).to(self.dev)
        self.omega, self.delta = torch.empty_like(self.lat), torch.empty_like(self.lat)
        with torch.cuda.device(self.dev):
            self.ws, self.ptr, self.nbytes = _workspace(self.lib, self.u0.shape, self.side, self.dev)
            check(self.lib.t2fit_n4_weights_dev(self.m.data_ptr(), *self.m.shape, self.side, self.omega.data_ptr(), self.ptr,
                                                self.nbytes, current_stream()))

    def histogram(self, lo, slope, bins):
        import torch

        with torch.cuda.device(self.dev):
            check(self.lib.t2fit_n4_histogram_dev(self.u.data_ptr(), self.m.data_ptr(), self.u.numel(), float(lo), float(slope),
                                                  int(bins), self.hist.data_ptr(), current_stream()))
            return self.hist[:bins].cpu().numpy().view(np.uint64)  # (waits)

    def fit(self, table, lo, slope):
        import torch

        bins = len(table)
        with torch.cuda.device(self.dev):
            self.table[:bins].copy_(torch.from_numpy(np.ascontiguousarray(table, np.float64)))
            check(self.lib.t2fit_n4_fit_dev(self.u.data_ptr(), self.m.data_ptr(), *self.u.shape, self.table.data_ptr(), float(lo),
                                            float(slope), bins, self.side, self.omega.data_ptr(), self.lat.data_ptr(),
                                            self.delta.data_ptr(), self.ptr, self.nbytes, current_stream()))

    def eval_field(self):
        import torch

        with torch.cuda.device(self.dev):
            check(self.lib.t2fit_n4_field_dev(self.lat.data_ptr(), self.side, self.u0.data_ptr(), self.m.data_ptr(), *self.u0.shape,
                                              self.field.data_ptr(), self.u.data_ptr(), self.sums.data_ptr(), self.rng.data_ptr(),
                                              self.ptr, self.nbytes, current_stream()))
            sums, rng = self.sums.cpu().numpy(), self.rng.cpu().numpy()  # (waits)
        return float(sums[0]), float(sums[1]), rng[0], rng[1]

    def lattice(self):
        return self.lat.cpu().numpy()

    def finish(self, scale):
        return apply_field(self.vol, self.field, scale), self.field


def n4_correct(volume_in, mask=None, *, fwhm=0.15, max_iter=_bias.DEFAULT_ITER, threshold=1e-3, bins=_bias.BINS, noise=0.01,
               scale=1.0, device=0):
    """N4 bias-field correction of a float32 ``(Z, Y, X)`` volume (numpy or CUDA tensor): what the reference asks of
    ``sitk.N4BiasFieldCorrectionImageFilter`` in ``run_biasfield_correction`` (utils/qmri_utils.py:254-357).  The log
    image inside ``mask`` (None: :func:`build_mask` on the device; voxels <= 0 are left out) is sharpened by deconvolving
    its 200-bin histogram with a Gaussian of full width ``fwhm`` (ITK's default 0.15; the reference uses 0.25 and 0.5),
    a cubic B-spline lattice is fitted to the difference, and that repeats until the field's change falls to
    ``threshold`` or ``max_iter[level]`` iterations, over lattices of side 4, 5, 7, 11 (one per entry of ``max_iter``, at
    most five).  Returns an :class:`N4Result`: ``corrected = volume / exp(log_field) * scale`` and ``log_field`` (numpy
    for numpy, tensors for a tensor), ``lattice``, ``iterations`` and ``convergence`` per level.  Every per-voxel pass
    runs on the GPU; iterations, lattice and field equal :func:`_bias.n4_correct`'s on the same log image.  Parity with
    ITK is unpinned."""
    import torch

    _bias.check_options(fwhm, max_iter, threshold, bins, noise, scale)
    dev = pick_device((volume_in, mask), device)
    v = volume(volume_in, torch.float32, dev)
    with torch.cuda.device(dev):
        m = build_mask(v, device=dev.index) if mask is None else mask
        found = _bias.n4_loop(DeviceSteps(v, m, dev), fwhm=fwhm, max_iter=max_iter, threshold=threshold, bins=bins, noise=noise,
                              scale=scale)
    found.corrected, found.log_field = _out(found.corrected, volume_in), _out(found.log_field, volume_in)
    return found
